// Source-filter split of the pitch path (pitchnorm.py): the spectral envelope of a frame of STFT
// magnitudes as its low-quefrency cepstrum, and the gain that warps that envelope along frequency by a per-row
// factor q while the harmonics stay where they are.  n_fft 400, 201 bins, w_k = 2 pi k / 400.  One kernel:
//   L[k]   = ln(max(S[k], floor_rel max_k S, 1e-10))
//   c_n    = (1 / 400) [L_0 + (-1)^n L_200 + 2 sum_{k = 1..199} L_k cos(2 pi n k / 400)],  n = 0..n_c
//   E(w)   = c_0 + 2 sum_{n = 1..n_c} c_n cos(n w)
//   g[k]   = clamp(E(min(pi, q w_k)) - E(w_k), +-max_gain_ln),   out[k] = S[k] exp(g[k])
// Plain fp32 FMAs (the cosines of the second sum by an fp64 recurrence), no atomics, the same bits on every run.
#include "sa_common.h"
#include <errno.h>

#define ENV_NFFT 400
#define ENV_NBIN 201
#define ENV_G 8                          // frames per workgroup
#define ENV_THREADS 256
#define ENV_NC_MAX 64
#define ENV_MAX_B 65535                  // grid.y
#define ENV_MAX_T (1 << 23)              // the vocoder's bound
#define ENV_TINY 1e-10f

typedef float f32x2 __attribute__((ext_vector_type(2)));
// two FMAs in one instruction (v_pk_fma_f32): the same bits as two fmaf
__device__ static inline f32x2 env_fma2(f32x2 a, float b, f32x2 c) {
  const f32x2 bb = {b, b};
  return __builtin_elementwise_fma(a, bb, c);
}

extern "C" int sa_env_dim(int which) {
  switch (which) {
    case 0: return ENV_NFFT;
    case 1: return ENV_NBIN;
    case 2: return ENV_G;
    case 3: return ENV_NC_MAX;
    case 4: return ENV_THREADS;
    default: return -EINVAL;
  }
}

__device__ static inline float env_q(float q) {            // a warp factor no kernel can be led astray by
  return q >= 0.25f && q <= 4.0f ? q : (q > 4.0f ? 4.0f : (q < 0.25f ? 0.25f : 1.0f));
}

// The store of stage (c) for one frame and bin: E(w_k) and E(theta_k) from the sums Ew and Et and the frame's c_0,
// the clamped gain, out = s exp(g) (at q == 1 a copy of s) and the optional env.
__device__ static inline void env_store(float Ew, float Et, float c0, float max_gain_ln, float q, float s, size_t o,
                                        float* __restrict__ out, float* __restrict__ env) {
  const float ew = fmaf(2.0f, Ew, c0), et = fmaf(2.0f, Et, c0);
  const float g = fminf(fmaxf(et - ew, -max_gain_ln), max_gain_ln);
  out[o] = q == 1.0f ? s : s * expf(g);
  if (env) env[o] = ew;
}

// grid (tiles of 8 frames, B), 4 waves.  The tile's 8 x 201 magnitudes are contiguous in memory and are staged as
// they lie.
//   (a) wave w takes the frames 2 w and 2 w + 1 and finds each frame's maximum by butterfly; then thread k forms L
//       of its bin for the eight frames and stores it as [k][frame], two 16-byte writes.
//   (b) thread (n, p) -- p in the low three bits -- sums its cepstral coefficient's terms at k = 1 + p + 8 j for
//       all eight frames at once: one cosine from a table of cos(2 pi i / 400) made in the kernel (fp64, rounded
//       once) and read at (n k) mod 400, which the thread steps by addition, feeds eight FMAs, and the eight L
//       arrive by two 16-byte reads (the eight p of a wave read one contiguous 256-byte line).  The eight partial
//       sums of an n meet by a butterfly over the three low lane bits -- a fixed order -- and the lane with p = 0
//       adds the two ends and stores the cepstra as [n][frame].
//   (c) thread k walks n once: the frames' eight c_n arrive by two 16-byte broadcast reads; cos(n w_k) and
//       cos(n theta_k) come from two Chebyshev recurrences in fp64 started at cospi, rounded to fp32 per term
//       (theta depends on (k, b) only, so one recurrence serves the eight frames); 2 x 8 fp32 accumulators.
// Frames from T on are staged as zeros and never stored.
// FRAMES (sa_env_warp_frames): qrow is [B][T], one factor per frame, and stage (c) runs one theta
// recurrence per frame instead of one per tile; everything else is the same text, and the per-frame accumulation is
// the fmaf the packed FMA is made of, so that a q constant along t gives sa_env_warp's bits.
template <bool FRAMES>
__global__ __launch_bounds__(ENV_THREADS) void sa_env_warp_kernel(const float* __restrict__ S,
                                                                  const float* __restrict__ qrow, int T, int n_c,
                                                                  float floor_rel, float max_gain_ln,
                                                                  float* __restrict__ out, float* __restrict__ env) {
  __shared__ float cs[ENV_NFFT];
  __shared__ float Ss[ENV_G * ENV_NBIN];
  __shared__ float fl[ENV_G];
  __shared__ __attribute__((aligned(16))) float Ls[ENV_NBIN * ENV_G];
  __shared__ __attribute__((aligned(16))) float cep[(ENV_NC_MAX + 1) * ENV_G];
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * ENV_G;
  const int nf = min(ENV_G, T - t0);                        // frames of this tile that exist
  const size_t base = ((size_t)b * T + t0) * ENV_NBIN;

  for (int i = tid; i < ENV_NFFT; i += ENV_THREADS) cs[i] = (float)cospi((double)i * (1.0 / 200.0));
  for (int e = tid; e < ENV_G * ENV_NBIN; e += ENV_THREADS) Ss[e] = e < nf * ENV_NBIN ? S[base + e] : 0.0f;
  __syncthreads();

  {  // (a)
    const int w = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float* row = Ss + (2 * w + h) * ENV_NBIN;
      float mx = 0.0f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = lane + 64 * j;
        mx = fmaxf(mx, k < ENV_NBIN ? row[k] : 0.0f);
      }
      mx = sa_wave_max(mx);
      if (lane == 0) fl[2 * w + h] = fmaxf(floor_rel * mx, ENV_TINY);
    }
  }
  __syncthreads();
  if (tid < ENV_NBIN) {
    f32x4 la, lb;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      la[f] = logf(fmaxf(Ss[f * ENV_NBIN + tid], fl[f]));
      lb[f] = logf(fmaxf(Ss[(4 + f) * ENV_NBIN + tid], fl[4 + f]));
    }
    *(f32x4*)(Ls + tid * ENV_G) = la;
    *(f32x4*)(Ls + tid * ENV_G + 4) = lb;
  }
  __syncthreads();

  // (b)
  for (int idx = tid; idx < (n_c + 1) * ENV_G; idx += ENV_THREADS) {
    const int n = idx >> 3, p = idx & 7;
    const int step = (8 * n) % ENV_NFFT;
    int i = (n * (1 + p)) % ENV_NFFT;                       // (n k) mod 400 at k = 1 + p
    f32x2 a2[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) a2[f] = (f32x2){0.0f, 0.0f};
    for (int k = 1 + p; k < ENV_NBIN - 1; k += 8) {
      const float c = cs[i];
      const f32x4 la = *(const f32x4*)(Ls + k * ENV_G), lb = *(const f32x4*)(Ls + k * ENV_G + 4);
      a2[0] = env_fma2(la.xy, c, a2[0]);
      a2[1] = env_fma2(la.zw, c, a2[1]);
      a2[2] = env_fma2(lb.xy, c, a2[2]);
      a2[3] = env_fma2(lb.zw, c, a2[3]);
      i += step;
      if (i >= ENV_NFFT) i -= ENV_NFFT;
    }
    float acc[ENV_G];
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[2 * f] = a2[f].x, acc[2 * f + 1] = a2[f].y;
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
#pragma unroll
      for (int f = 0; f < ENV_G; ++f) acc[f] += __shfl_xor(acc[f], o, 64);
    }
    if (p == 0) {
      f32x4 ca, cb;
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const float e0 = Ls[f], e1 = Ls[(ENV_NBIN - 1) * ENV_G + f];
        const float g0 = Ls[4 + f], g1 = Ls[(ENV_NBIN - 1) * ENV_G + 4 + f];
        ca[f] = fmaf(2.0f, acc[f], (n & 1) ? e0 - e1 : e0 + e1) / (float)ENV_NFFT;
        cb[f] = fmaf(2.0f, acc[4 + f], (n & 1) ? g0 - g1 : g0 + g1) / (float)ENV_NFFT;
      }
      *(f32x4*)(cep + n * ENV_G) = ca;
      *(f32x4*)(cep + n * ENV_G + 4) = cb;
    }
  }
  __syncthreads();

  // (c)
  const int k = tid;
  if (k >= ENV_NBIN) return;
  if constexpr (FRAMES) {
    const double wk = (double)k * (1.0 / 200.0);            // w_k / pi
    const double xw = cospi(wk), xw2 = 2.0 * xw;
    float qf[ENV_G];
    double h0[ENV_G], h1[ENV_G], xt2[ENV_G];
    float Ew[ENV_G], Et[ENV_G];
#pragma unroll
    for (int f = 0; f < ENV_G; ++f) {
      qf[f] = env_q(f < nf ? qrow[(size_t)b * T + t0 + f] : 1.0f);
      const double xt = cospi(fmin(1.0, (double)qf[f] * wk));
      h0[f] = 1.0, h1[f] = xt, xt2[f] = 2.0 * xt;
      Ew[f] = Et[f] = 0.0f;
    }
    double w0 = 1.0, w1 = xw;
    for (int n = 1; n <= n_c; ++n) {
      const float cw = (float)w1;
      const f32x4 ca = *(const f32x4*)(cep + n * ENV_G), cb = *(const f32x4*)(cep + n * ENV_G + 4);
#pragma unroll
      for (int f = 0; f < ENV_G; ++f) {
        const float cf = f < 4 ? ca[f & 3] : cb[f & 3];
        const float ct = (float)h1[f];
        Ew[f] = fmaf(cf, cw, Ew[f]), Et[f] = fmaf(cf, ct, Et[f]);
        const double h2 = fma(xt2[f], h1[f], -h0[f]);
        h0[f] = h1[f], h1[f] = h2;
      }
      const double w2 = fma(xw2, w1, -w0);
      w0 = w1, w1 = w2;
    }
#pragma unroll
    for (int f = 0; f < ENV_G; ++f)
      if (f < nf)
        env_store(Ew[f], Et[f], cep[f], max_gain_ln, qf[f], Ss[f * ENV_NBIN + k], base + (size_t)f * ENV_NBIN + k,
                  out, env);
    return;
  }
  const float q = env_q(qrow[b]);
  const double wk = (double)k * (1.0 / 200.0);              // w_k / pi
  const double xw = cospi(wk), xt = cospi(fmin(1.0, (double)q * wk));
  double w0 = 1.0, w1 = xw, h0 = 1.0, h1 = xt;              // cos((n - 1) .), cos(n .)
  f32x2 Ew2[4], Et2[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) Ew2[f] = Et2[f] = (f32x2){0.0f, 0.0f};
  const double xw2 = 2.0 * xw, xt2 = 2.0 * xt;
  for (int n = 1; n <= n_c; ++n) {
    const float cw = (float)w1, ct = (float)h1;
    const f32x4 ca = *(const f32x4*)(cep + n * ENV_G), cb = *(const f32x4*)(cep + n * ENV_G + 4);
    Ew2[0] = env_fma2(ca.xy, cw, Ew2[0]), Et2[0] = env_fma2(ca.xy, ct, Et2[0]);
    Ew2[1] = env_fma2(ca.zw, cw, Ew2[1]), Et2[1] = env_fma2(ca.zw, ct, Et2[1]);
    Ew2[2] = env_fma2(cb.xy, cw, Ew2[2]), Et2[2] = env_fma2(cb.xy, ct, Et2[2]);
    Ew2[3] = env_fma2(cb.zw, cw, Ew2[3]), Et2[3] = env_fma2(cb.zw, ct, Et2[3]);
    const double w2 = fma(xw2, w1, -w0), h2 = fma(xt2, h1, -h0);
    w0 = w1, w1 = w2, h0 = h1, h1 = h2;
  }
  float Ew[ENV_G], Et[ENV_G];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    Ew[2 * f] = Ew2[f].x, Ew[2 * f + 1] = Ew2[f].y;
    Et[2 * f] = Et2[f].x, Et[2 * f + 1] = Et2[f].y;
  }
#pragma unroll
  for (int f = 0; f < ENV_G; ++f)
    if (f < nf)
      env_store(Ew[f], Et[f], cep[f], max_gain_ln, q, Ss[f * ENV_NBIN + k], base + (size_t)f * ENV_NBIN + k, out,
                env);
}

static inline bool env_args_ok(const float* S, const float* q, int B, int T, int n_c, float floor_rel,
                               float max_gain_ln, const float* out) {
  return S && q && out && B >= 1 && B <= ENV_MAX_B && T >= 1 && T <= ENV_MAX_T && n_c >= 1 && n_c <= ENV_NC_MAX &&
         floor_rel > 0.0f && floor_rel < 1.0f && max_gain_ln > 0.0f;          // (a NaN fails its comparison)
}

extern "C" int sa_env_warp(const float* S, const float* q, int B, int T, int n_c, float floor_rel, float max_gain_ln,
                           float* out, float* env, void* stream) {
  if (!env_args_ok(S, q, B, T, n_c, floor_rel, max_gain_ln, out)) return -EINVAL;
  hipLaunchKernelGGL(sa_env_warp_kernel<false>, dim3(sa_div_up(T, ENV_G), B), dim3(ENV_THREADS), 0,
                     (hipStream_t)stream, S, q, T, n_c, floor_rel, max_gain_ln, out, env);
  return -(int)hipGetLastError();
}

extern "C" int sa_env_warp_frames(const float* S, const float* q, int B, int T, int n_c, float floor_rel,
                                  float max_gain_ln, float* out, float* env, void* stream) {
  if (!env_args_ok(S, q, B, T, n_c, floor_rel, max_gain_ln, out)) return -EINVAL;
  hipLaunchKernelGGL(sa_env_warp_kernel<true>, dim3(sa_div_up(T, ENV_G), B), dim3(ENV_THREADS), 0,
                     (hipStream_t)stream, S, q, T, n_c, floor_rel, max_gain_ln, out, env);
  return -(int)hipGetLastError();
}
