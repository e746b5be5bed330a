// LPC formant tracking and its comparison (ops.formant_tracks, ops.formant_compare; DESIGN section 25;
// include/sa_hip.h carries the definition).  Per frame of 400 samples at hop 160 (the frame grid of the F0 tracks:
// frame t covers [160 t - 200, 160 t + 200)), pre-emphasised and under the Hamming window, in fp64:
//   e[n] = x[n] - 0.97 x[n - 1];  f = w e;  r_k = sum_j f[j] f[j + k], k = 0..18;  r_0 < 1e-10: silent (status 1)
//   r_0 *= 1 + 1e-9;  a = Levinson-Durbin(r);  some |k_i| >= 1 or an error <= 0: fallback (status 2)
//   z = the 18 roots of a by Aberth-Ehrlich, one lane per root, at most 64 iterations, stop under 1e-14; no
//       convergence: fallback
//   candidates: Im z > 1e-6 |z|, f = arg z 16000 / 2 pi, b = -ln|z| 16000 / pi, kept when 90 <= f <= 5500 and b <= 700
//   fewer than three kept: short (status 3); otherwise F1..F3 and their bandwidths are the three of lowest f
// sa_formant_compare: over the frames scored and voiced in both signals, the lower medians of the degraded track and
// of the per-frame ratios, and the geometric mean of the three ratios; the medians by a bitwise radix select.
// The fit and the root finder are sa_lpc_shared.h's at order 18, the select's helpers too.
// No atomics, every sum in a fixed order: the same bits on every run.
#include "sa_lpc_shared.h"

#define FT_W 400
#define FT_H 160
#define FT_P 18
#define FT_NF 3
#define FT_THREADS 64
#define FT_PART 147                      // samples per part of a lag sum: 147 mod 32 = 19 (the LDS banks, below)
#define FT_MAX_B 65535                   // grid.y
#define FT_MAX_N (1 << 24)
#define FT_MAX_T 104858                  // the frames of 2^24 samples
#define FT_FMIN 90.0
#define FT_FMAX 5500.0
#define FT_BMAX 700.0
#define FT_HZ_PER_RAD 2546.4790894703255  // 16000 / 2 pi
#define FT_BW_PER_NEPER 5092.958178940651 // 16000 / pi
#define FC_THREADS 1024
#define FC_WAVES (FC_THREADS / 64)
#define FC_SEL (2 * FT_NF)               // three medians of the track, three of the ratios

extern "C" int sa_formant_dim(int which) {
  switch (which) {
    case 0: return FT_W;
    case 1: return FT_H;
    case 2: return FT_P;
    case 3: return FT_NF;
    case 4: return FT_THREADS;
    case 5: return SA_LPC_ITERS;
    case 6: return FT_MAX_T;
    case 7: return FC_THREADS;
    default: return -EINVAL;
  }
}

// grid (T, B), one wave.  LDS: the windowed frame as fp64 with 18 zeros behind it, so that the lag sums read zeros
// past the far end instead of branching.
//   (a) lane j mod 64 pre-emphasises and windows seven samples (six in the lanes from 16 on)
//   (b) lane (k, part) sums lag k over a part of 147 samples (the third part: 106); the three parts are added in
//       order.  By the bank rule of ds_read_b64 (bank = (a / 4) mod 64, conflicts within a 32-lane half): the lanes of
//       a part read f[j] at one address (a broadcast) and f[j + k] at 19 consecutive doubles; two parts share a half
//       and lie 147 doubles = 19 mod 32 apart, so their 19 + 13 (6 + 19 in the upper half) doubles fall into
//       different banks of the 32-double row
//   (c) every lane runs the Levinson recursion on the same values, fully unrolled in registers
//   (d) lane j < 18 owns root j: Horner for p and p', the Aberth sum over the other 17 by lane reads
//   (e) lane j judges its root; each kept lane counts the kept lanes of lower frequency, ranks 0, 1, 2 write
__global__ __launch_bounds__(FT_THREADS) void sa_formant_tracks_kernel(const float* __restrict__ wav,
                                                                       const int* __restrict__ n_valid, int N, int T,
                                                                       float* __restrict__ freq,
                                                                       float* __restrict__ bw,
                                                                       int* __restrict__ status) {
  __shared__ double fs[FT_W + FT_P];
  __shared__ double part[FT_THREADS];
  const int lane = threadIdx.x, t = blockIdx.x, b = blockIdx.y;
  const int nv = min(max(n_valid[b], 0), N);
  const float* x = wav + (size_t)b * N;

  // (a)
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int j = lane + 64 * i, n = FT_H * t - FT_W / 2 + j;
    if (j < FT_W) {
      double e = 0.0;
      if (n >= 0 && n < nv) {
        const double prev = n >= 1 ? (double)x[n - 1] : 0.0;
        e = (double)x[n] - __dmul_rn(0.97, prev);
      }
      const double w = 0.54 - __dmul_rn(0.46, cospi((double)j * (2.0 / 399.0)));
      fs[j] = w * e;
    }
  }
  if (lane < FT_P) fs[FT_W + lane] = 0.0;
  __syncthreads();

  // (b), (c)
  double a[FT_P + 1], unused;
  int st = sa_lpc_fit<FT_P, FT_W, FT_PART, 0>(fs, part, lane, a, unused);

  double fz = 0.0, bz = 0.0;
  bool kept = false;
  if (st == 0) {
    // (d)
    const bool mine = lane < FT_P;
    double zr, zi;
    const bool conv = sa_lpc_aberth<FT_P>(a, lane, zr, zi);
    if (!conv) st = 2;

    if (st == 0) {
      // (e)
      const double mod = sqrt(fma(zr, zr, zi * zi));
      fz = atan2(zi, zr) * FT_HZ_PER_RAD;
      bz = -log(mod) * FT_BW_PER_NEPER;
      kept = mine && zi > SA_LPC_REAL * mod && fz >= FT_FMIN && fz <= FT_FMAX && bz <= FT_BMAX;
      if (__popcll(__ballot(kept)) < FT_NF) st = 3;
    }
  }

  const size_t row = (size_t)b * T + t;
  if (st == 0) {
    int rank = 0;
#pragma unroll
    for (int k = 0; k < FT_P; ++k) {
      const double fk = __shfl(fz, k, 64);
      const bool kk = __shfl((int)kept, k, 64) != 0;
      rank += kk && (fk < fz || (fk == fz && k < lane));
    }
    if (kept && rank < FT_NF) {
      freq[row * FT_NF + rank] = (float)fz;
      if (bw) bw[row * FT_NF + rank] = (float)bz;
    }
  } else if (lane < FT_NF) {
    freq[row * FT_NF + lane] = 0.0f;
    if (bw) bw[row * FT_NF + lane] = 0.0f;
  }
  if (status && lane == 0) status[row] = st;
}

extern "C" int sa_formant_tracks(const float* wav, const int* n_valid, int B, int N, float* freq, float* bw,
                                 int* status, void* stream) {
  if (!wav || !n_valid || !freq || B < 1 || B > FT_MAX_B || N < 1 || N > FT_MAX_N) return -EINVAL;
  const int T = N / FT_H + 1;
  hipLaunchKernelGGL(sa_formant_tracks_kernel, dim3(T, B), dim3(FT_THREADS), 0, (hipStream_t)stream, wav, n_valid, N, T,
                     freq, bw, status);
  return -(int)hipGetLastError();
}

// ---- comparison ----------------------------------------------------------------------------------------
// (the key, its inverse and the workgroup count of the select: sa_lpc_shared.h)
// grid B, one workgroup of 16 waves per row; thread i takes the frames i, i + 1024, ...  A first pass counts the frames
// that count; then 32 passes, one per bit of the key from the top, settle that bit of all six medians at once: the
// frames whose key agrees with the bits settled so far and has a 0 at this one are counted, and the rank sought lies
// among them or past them.  One path for every T; the tracks are read 33 times, from the caches after the first.
__global__ __launch_bounds__(FC_THREADS) void sa_formant_compare_kernel(
    const float* __restrict__ F_ref, const float* __restrict__ F_deg, const int* __restrict__ st_ref,
    const int* __restrict__ st_deg, const float* __restrict__ f0_ref, const float* __restrict__ f0_deg,
    const int* __restrict__ frames, int T, int min_common, float* __restrict__ med, float* __restrict__ ratio,
    float* __restrict__ shift, int* __restrict__ common) {
  __shared__ int cnt[2][FC_WAVES][FC_SEL];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int F = min(max(frames[b], 0), T);
  const size_t base = (size_t)b * T;
  const float* Fr = F_ref + base * FT_NF;
  const float* Fd = F_deg + base * FT_NF;
  const int *sr = st_ref + base, *sd = st_deg + base;
  const float *pr = f0_ref + base, *pd = f0_deg + base;

  int c[FC_SEL];
#pragma unroll
  for (int s = 0; s < FC_SEL; ++s) c[s] = 0;
  for (int t = tid; t < F; t += FC_THREADS)
    c[0] += sr[t] == 0 && sd[t] == 0 && pr[t] > 0.0f && pd[t] > 0.0f;
  sa_sel_block_sum(c, cnt, 0);
  const int n = c[0];
  const bool scored = n >= min_common;                      // (uniform)

  unsigned prefix[FC_SEL];
  int want[FC_SEL];
#pragma unroll
  for (int s = 0; s < FC_SEL; ++s) prefix[s] = 0u, want[s] = (n - 1) / 2;
  if (scored) {
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned one = 1u << bit, mask = ~(one - 1u);   // the bits settled so far, and this one
#pragma unroll
      for (int s = 0; s < FC_SEL; ++s) c[s] = 0;
      for (int t = tid; t < F; t += FC_THREADS) {
        if (sr[t] == 0 && sd[t] == 0 && pr[t] > 0.0f && pd[t] > 0.0f) {
#pragma unroll
          for (int k = 0; k < FT_NF; ++k) {
            const float d = Fd[(size_t)t * FT_NF + k], g = Fr[(size_t)t * FT_NF + k];
            const float q = (float)((double)d / (double)g);
            c[k] += (sa_sel_key(d) & mask) == prefix[k];
            c[FT_NF + k] += (sa_sel_key(q) & mask) == prefix[FT_NF + k];
          }
        }
      }
      sa_sel_block_sum(c, cnt, bit & 1);                        // (31 -> 1 after the count's 0, then alternating)
#pragma unroll
      for (int s = 0; s < FC_SEL; ++s)
        if (want[s] >= c[s]) want[s] -= c[s], prefix[s] |= one;
    }
  }
  if (tid != 0) return;
  float m[FT_NF], q[FT_NF];
  double lg = 0.0;
#pragma unroll
  for (int k = 0; k < FT_NF; ++k) {
    m[k] = scored ? sa_sel_value(prefix[k]) : 0.0f;
    q[k] = scored ? sa_sel_value(prefix[FT_NF + k]) : 0.0f;
    lg += log((double)q[k]);
  }
#pragma unroll
  for (int k = 0; k < FT_NF; ++k) {
    if (med) med[(size_t)b * FT_NF + k] = m[k];
    if (ratio) ratio[(size_t)b * FT_NF + k] = q[k];
  }
  shift[b] = scored ? (float)exp(lg / 3.0) : 0.0f;
  if (common) common[b] = scored ? n : 0;
}

extern "C" int sa_formant_compare(const float* F_ref, const float* F_deg, const int* st_ref, const int* st_deg,
                                  const float* f0_ref, const float* f0_deg, const int* frames, int B, int T,
                                  int min_common, float* med, float* ratio, float* shift, int* common, void* stream) {
  if (!F_ref || !F_deg || !st_ref || !st_deg || !f0_ref || !f0_deg || !frames || !shift || B < 1 || B > FT_MAX_B ||
      T < 1 || T > FT_MAX_T || min_common < 1)
    return -EINVAL;
  hipLaunchKernelGGL(sa_formant_compare_kernel, dim3(B), dim3(FC_THREADS), 0, (hipStream_t)stream, F_ref, F_deg, st_ref,
                     st_deg, f0_ref, f0_deg, frames, T, min_common, med, ratio, shift, common);
  return -(int)hipGetLastError();
}
