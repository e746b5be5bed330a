// x-vector gender classifier in TRAIN mode (the recipe of gender_classifier_train.py: Xvector +
// Classifier trained with NLL, BatchNorm on batch statistics).  Five TDNN blocks
//   z = LeakyReLU(conv_same_reflect(x) + bias),  y = BN_train(z) = s*z + t
// with activations [B][T][C] (fp32), split-bf16 MFMA operands on both sides, fp32 accumulation and
// fp64 statistics finalisers (sa_sum_partials / sa_fin_bn_fwd / sa_fin_norm_bwd / sa_fin_bias).
// Nothing here uses float atomics: every reduction is written as fixed-order partials and added in
// a fixed order, so a step gives the same bits on every run.
//   sa_xv_tdnn_fwd_train   z and per-(utterance, 128-frame tile) partials of sum z, sum z^2; the
//                          previous block's BatchNorm affine is applied to the input while staging
//   sa_xv_colsums          per-channel fp64 partials over row chunks of a [M][N] matrix (batch
//                          statistics, BatchNorm backward sums) and, with the folded coefficients,
//                          the pre-activation gradient dpre = leak'(z) * (c1*dy + c2*z + c3)
//   sa_xv_tdnn_wgrad       dW_k = dpre^T x_k over the B*T rows, split across workgroups
//   sa_xv_wgrad_reduce     the split partials added in split order, into the torch [Cout][Cin][K] layout
//   sa_xv_tdnn_dgrad       d x (extended range) = sum_k W_k^T dpre, then sa_tdnn_fold
//   sa_xv_pool_affine(_bwd) statistics pooling of y = s*z + t from the pooled statistics of z
#include "sa_common.h"
#include "../../include/sa_hip.h"

#define SA_XT_BM 128                      // frames per workgroup (forward / data gradient)
#define SA_XT_BN 128                      // output channels per workgroup
#define SA_XT_CK 64                       // reduction channels per LDS chunk
#define SA_XT_HALO 8                      // >= dil*(K-1) for the x-vector layers
#define SA_XT_RK 32                       // rows per LDS stage of the weight gradient

static inline int sa_xt_reflect_ok(int T, int K, int dil) {
  return K >= 1 && (K & 1) && dil >= 1 && dil * (K - 1) / 2 < T && dil * (K - 1) <= SA_XT_HALO;
}

// ---------------------------------------------------------------------------------
// train-mode forward: sa_tdnn_fwd_kernel's tiling (128 frames x 128 channels of one utterance per
// 4-wave workgroup, input channels through LDS in chunks of 64 with the reflect halo, weights as the
// SA_BF16X3 fragment image from L2).  Prologue: x = s_in*x + t_in per input channel (the previous
// block's BatchNorm; none for block 0).  Epilogue: z = leaky(acc + bias) stored, and
// part[b*ntile + tile][n][0..1] = (sum z, sum z^2) over the tile's valid frames (fp32, fixed order:
// the two half-waves, then the two waves that share the columns).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void sa_xv_tdnn_fwd_train_kernel(
    const float* __restrict__ x, const float* __restrict__ s_in, const float* __restrict__ t_in,
    const bf16x8* __restrict__ wp, const float* __restrict__ bias, float* __restrict__ z,
    float* __restrict__ part, int T, int Cin, int Cout, int Npad, int K, int dil, float slope) {
  constexpr int PITCH = SA_XT_CK + 8, ROWS = SA_XT_BM + SA_XT_HALO, PLANE = ROWS * PITCH;
  __shared__ __attribute__((aligned(16))) bf16_t As[2 * PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int t0 = blockIdx.x * SA_XT_BM, n0 = blockIdx.y * SA_XT_BN, b = blockIdx.z;
  const int pad = dil * (K - 1) / 2, nrows = SA_XT_BM + 2 * pad;
  const int KSTEPS = Cin / 16, NT = Npad / 32;
  const size_t lo_off = (size_t)K * KSTEPS * NT * 64;
  f32x16 acc[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0.0f;
  const float* xb = x + (size_t)b * T * Cin;
  for (int c0 = 0; c0 < Cin; c0 += SA_XT_CK) {
    const int ck = Cin - c0 < SA_XT_CK ? Cin - c0 : SA_XT_CK, chunks = ck / 4;
    for (int e = tid; e < nrows * chunks; e += 256) {
      const int r = e / chunks, c = e % chunks, ch = c0 + c * 4;
      int tt = t0 + r - pad;
      if (tt < 0) tt = -tt;
      if (tt >= T) tt = 2 * (T - 1) - tt;
      float f[4] = {0.f, 0.f, 0.f, 0.f};
      if (tt >= 0 && tt < T) {
        const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)tt * Cin + ch);
        f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
        if (s_in) {
#pragma unroll
          for (int j = 0; j < 4; ++j) f[j] = fmaf(s_in[ch + j], f[j], t_in[ch + j]);
        }
      }
      uint2 hi, lo;
      sa_split4(f, hi, lo);
      *reinterpret_cast<uint2*>(As + r * PITCH + c * 4) = hi;
      *reinterpret_cast<uint2*>(As + PLANE + r * PITCH + c * 4) = lo;
    }
    __syncthreads();
    const int ksteps = ck / 16;
    for (int k = 0; k < K; ++k) {
      for (int ks = 0; ks < ksteps; ++ks) {
        const bf16x8* wt = wp + (((size_t)k * KSTEPS + c0 / 16 + ks) * NT + n0 / 32 + wn * 2) * 64 + lane;
        bf16x8 bh[2], bl[2], ah[2], al[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) { bh[nt] = wt[nt * 64]; bl[nt] = wt[lo_off + nt * 64]; }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          const bf16_t* ap = As + (wm * 64 + mt * 32 + (lane & 31) + k * dil) * PITCH + ks * 16 + 8 * (lane >> 5);
          ah[mt] = *reinterpret_cast<const bf16x8*>(ap);
          al[mt] = *reinterpret_cast<const bf16x8*>(ap + PLANE);
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) {
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mt], bh[nt], acc[mt][nt], 0, 0, 0);
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bl[nt], acc[mt][nt], 0, 0, 0);
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bh[nt], acc[mt][nt], 0, 0, 0);
          }
      }
    }
    __syncthreads();
  }
  float* red = reinterpret_cast<float*>(As);           // [2 waves along frames][128 columns][2]
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int nl = (wn * 2 + nt) * 32 + (lane & 31), n = n0 + nl;
    float s = 0.0f, q = 0.0f;
    if (n < Cout) {
      const float bb = bias ? bias[n] : 0.0f;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int t = t0 + wm * 64 + mt * 32 + sa_acc_row(i, lane);
          if (t < T) {
            float v = acc[mt][nt][i] + bb;
            v = v > 0.0f ? v : v * slope;
            z[((size_t)b * T + t) * Cout + n] = v;
            s += v; q = fmaf(v, v, q);
          }
        }
    }
    s += __shfl_xor(s, 32, 64);
    q += __shfl_xor(q, 32, 64);
    if (lane < 32) { red[(wm * 128 + nl) * 2] = s; red[(wm * 128 + nl) * 2 + 1] = q; }
  }
  __syncthreads();
  if (tid < SA_XT_BN && n0 + tid < Cout) {
    float* o = part + (((size_t)b * gridDim.x + blockIdx.x) * Cout + n0 + tid) * 2;
    o[0] = red[tid * 2] + red[(128 + tid) * 2];
    o[1] = red[tid * 2 + 1] + red[(128 + tid) * 2 + 1];
  }
}

extern "C" int sa_xv_tdnn_fwd_train(const float* x, const float* s_in, const float* t_in, const void* wp,
                                    const float* bias, float* z, float* part, int B, int T, int Cin, int Cout,
                                    int Npad, int K, int dil, float slope, void* stream) {
  if (!x || !wp || !z || !part || B <= 0 || T <= 0 || Cin <= 0 || Cout <= 0 || (!s_in) != (!t_in) ||
      !sa_xt_reflect_ok(T, K, dil) || Cin % 16 || Npad % SA_XT_BN || Npad < Cout)
    return -22;
  dim3 grid(sa_div_up(T, SA_XT_BM), Npad / SA_XT_BN, B);
  hipLaunchKernelGGL(sa_xv_tdnn_fwd_train_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x,
                     s_in, t_in, reinterpret_cast<const bf16x8*>(wp), bias, z, part, T, Cin, Cout, Npad, K, dil,
                     slope);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

extern "C" int sa_xv_tdnn_ntiles(int T) { return T > 0 ? sa_div_up(T, SA_XT_BM) : 0; }

// ---------------------------------------------------------------------------------
// column statistics of G [M][N] over row chunks of `rows_per` rows, fp64, fixed order (4 row lanes
// per column, added in lane order): part[chunk][n] = (sum v, sum v*h) with
//   v = G                                           (c1 == null)
//   v = (c1*G + c2*H + c3) * (H > 0 ? 1 : slope)    (c1 != null; v also stored to `out`)
//   h = H (or v when H == null), normalised (h - hmean)*hrstd when hmean != null.
// Uses: batch statistics (G = z), BatchNorm backward sums (G = dy, H = z, hmean/hrstd), the
// pre-activation gradient with its bias sums (G = dy, H = z, folded coefficients).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sa_xv_colsums_kernel(const float* __restrict__ G, const float* __restrict__ H,
                                                            const float* __restrict__ hm, const float* __restrict__ hr,
                                                            const float* __restrict__ c1, const float* __restrict__ c2,
                                                            const float* __restrict__ c3, float slope,
                                                            float* __restrict__ out, int M, int N, int rows_per,
                                                            double* __restrict__ part) {
  __shared__ double red[4][64][2];
  const int cl = threadIdx.x & 63, q = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
  const int r0 = blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
  double s = 0.0, p = 0.0;
  if (c < N) {
    const float k1 = c1 ? c1[c] : 0.0f, k2 = c1 ? c2[c] : 0.0f, k3 = c1 ? c3[c] : 0.0f;
    const float mh = hm ? hm[c] : 0.0f, rh = hm ? hr[c] : 1.0f;
    for (int r = r0 + q; r < r1; r += 4) {
      const size_t i = (size_t)r * N + c;
      float v = G[i];
      float h = H ? H[i] : v;
      if (c1) {
        v = fmaf(k1, v, fmaf(k2, h, k3)) * (h > 0.0f ? 1.0f : slope);
        out[i] = v;
        if (!H) h = v;
      }
      if (hm) h = (h - mh) * rh;
      s += (double)v;
      p += (double)v * (double)h;
    }
  }
  red[q][cl][0] = s; red[q][cl][1] = p;
  __syncthreads();
  if (q == 0 && c < N) {
    double a = red[0][cl][0], bq = red[0][cl][1];
#pragma unroll
    for (int k = 1; k < 4; ++k) { a += red[k][cl][0]; bq += red[k][cl][1]; }
    part[((size_t)blockIdx.y * N + c) * 2] = a;
    part[((size_t)blockIdx.y * N + c) * 2 + 1] = bq;
  }
}

extern "C" int sa_xv_colsums(const float* G, const float* H, const float* hmean, const float* hrstd,
                             const float* c1, const float* c2, const float* c3, float slope, float* out, int M,
                             int N, int rows_per, double* part, void* stream) {
  if (!G || !part || M <= 0 || N <= 0 || rows_per <= 0 || (hmean && !hrstd) || (c1 && (!c2 || !c3 || !out)))
    return -22;
  dim3 grid(sa_div_up(N, 64), sa_div_up(M, rows_per));
  hipLaunchKernelGGL(sa_xv_colsums_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), G, H,
                     hmean, hrstd, c1, c2, c3, slope, out, M, N, rows_per, part);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

// ---------------------------------------------------------------------------------
// TDNN weight gradient.  For tap k (offset o_k = k*dil - pad):
//   part[split][k][co][ci] = sum_{r in split} dpre[r][co] * x'[b, refl(t + o_k), ci],   r = b*T + t
// x' = s_in*x + t_in (the previous block's BatchNorm, none for block 0).  GEMM with M = Cout,
// N = Cin and the reduction over the rows: both operands are [rows][channels], so they are staged
// TRANSPOSED into LDS ([channel][row], rows contiguous; two rows per 32-bit store), split hi / lo,
// and read as the MFMA's 8-consecutive-K fragments.  One 4-wave workgroup = 128 co x 128 ci of one
// tap over `rows_per` rows (32 per LDS stage); the splits are added by sa_xv_wgrad_reduce in split
// order (deterministic; no atomics).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void sa_xv_tdnn_wgrad_kernel(
    const float* __restrict__ dpre, const float* __restrict__ x, const float* __restrict__ s_in,
    const float* __restrict__ t_in, float* __restrict__ part, int M, int T, int Cin, int Cout, int K, int dil,
    int rows_per) {
  constexpr int P = SA_XT_RK + 8, PLANE = 128 * P;
  __shared__ __attribute__((aligned(16))) bf16_t As[2 * PLANE];
  __shared__ __attribute__((aligned(16))) bf16_t Bs[2 * PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int co0 = blockIdx.x * 128, k = blockIdx.y % K, ci0 = (blockIdx.y / K) * 128;
  const int off = k * dil - dil * (K - 1) / 2;
  const int rb = blockIdx.z * rows_per, re = min(M, rb + rows_per);
  f32x16 acc[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0.0f;
  for (int r0 = rb; r0 < re; r0 += SA_XT_RK) {
    // 16 row pairs x 32 channel quads; 8 quads of a row are neighbours in a wave (128-byte reads)
    for (int e = tid; e < 512; e += 256) {
      const int q = ((e >> 7) << 3) | (e & 7), pr = (e >> 3) & 15;
      float fa[2][4], fb[2][4];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = r0 + 2 * pr + j, co = co0 + 4 * q, ci = ci0 + 4 * q;
#pragma unroll
        for (int c = 0; c < 4; ++c) { fa[j][c] = 0.0f; fb[j][c] = 0.0f; }
        if (r < re && co < Cout) {
          const float4 v = *reinterpret_cast<const float4*>(dpre + (size_t)r * Cout + co);
          fa[j][0] = v.x; fa[j][1] = v.y; fa[j][2] = v.z; fa[j][3] = v.w;
        }
        if (r < re && ci < Cin) {
          const int b = r / T;
          int tt = r - b * T + off;
          if (tt < 0) tt = -tt;
          if (tt >= T) tt = 2 * (T - 1) - tt;
          const float4 v = *reinterpret_cast<const float4*>(x + ((size_t)b * T + tt) * Cin + ci);
          fb[j][0] = v.x; fb[j][1] = v.y; fb[j][2] = v.z; fb[j][3] = v.w;
          if (s_in) {
#pragma unroll
            for (int c = 0; c < 4; ++c) fb[j][c] = fmaf(s_in[ci + c], fb[j][c], t_in[ci + c]);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bf16_t ah0 = (bf16_t)fa[0][c], ah1 = (bf16_t)fa[1][c];
        const bf16_t al0 = (bf16_t)(fa[0][c] - (float)ah0), al1 = (bf16_t)(fa[1][c] - (float)ah1);
        const bf16_t bh0 = (bf16_t)fb[0][c], bh1 = (bf16_t)fb[1][c];
        const bf16_t bl0 = (bf16_t)(fb[0][c] - (float)bh0), bl1 = (bf16_t)(fb[1][c] - (float)bh1);
        const int at = (4 * q + c) * P + 2 * pr;
        bf16_t* a = As + at;
        bf16_t* bp = Bs + at;
        a[0] = ah0; a[1] = ah1; a[PLANE] = al0; a[PLANE + 1] = al1;
        bp[0] = bh0; bp[1] = bh1; bp[PLANE] = bl0; bp[PLANE + 1] = bl1;
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < SA_XT_RK / 16; ++ks) {
      bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const bf16_t* ap = As + (wm * 64 + mt * 32 + (lane & 31)) * P + ks * 16 + 8 * (lane >> 5);
        ah[mt] = *reinterpret_cast<const bf16x8*>(ap);
        al[mt] = *reinterpret_cast<const bf16x8*>(ap + PLANE);
      }
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const bf16_t* bp = Bs + (wn * 64 + nt * 32 + (lane & 31)) * P + ks * 16 + 8 * (lane >> 5);
        bh[nt] = *reinterpret_cast<const bf16x8*>(bp);
        bl[nt] = *reinterpret_cast<const bf16x8*>(bp + PLANE);
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mt], bh[nt], acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bl[nt], acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bh[nt], acc[mt][nt], 0, 0, 0);
        }
    }
    __syncthreads();
  }
  float* o = part + ((size_t)blockIdx.z * K + k) * Cout * Cin;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int ci = ci0 + wn * 64 + nt * 32 + (lane & 31);
    if (ci < Cin) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int co = co0 + wm * 64 + mt * 32 + sa_acc_row(i, lane);
          if (co < Cout) o[(size_t)co * Cin + ci] = acc[mt][nt][i];
        }
    }
  }
}

extern "C" int sa_xv_tdnn_wgrad(const float* dpre, const float* x, const float* s_in, const float* t_in,
                                float* part, int B, int T, int Cin, int Cout, int K, int dil, int nsplit,
                                int rows_per, void* stream) {
  if (!dpre || !x || !part || B <= 0 || T <= 0 || Cin <= 0 || Cout <= 0 || Cin % 4 || Cout % 4 ||
      (!s_in) != (!t_in) || !sa_xt_reflect_ok(T, K, dil) || nsplit <= 0 || rows_per <= 0 ||
      rows_per % SA_XT_RK || (long long)nsplit * rows_per < (long long)B * T)
    return -22;
  dim3 grid(sa_div_up(Cout, 128), sa_div_up(Cin, 128) * K, nsplit);
  hipLaunchKernelGGL(sa_xv_tdnn_wgrad_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), dpre, x,
                     s_in, t_in, part, B * T, T, Cin, Cout, K, dil, rows_per);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

// dW[co][ci][k] = sum_split part[split][k][co][ci], fp64, in split order
__global__ void sa_xv_wgrad_reduce_kernel(const float* __restrict__ part, int nsplit, int K, int Cout, int Cin,
                                          float* __restrict__ dW) {
  const size_t n = (size_t)K * Cout * Cin;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int k = (int)(i % K);
  const size_t oc = i / K;                           // co*Cin + ci
  double s = 0.0;
  for (int sp = 0; sp < nsplit; ++sp) s += (double)part[((size_t)sp * K + k) * Cout * Cin + oc];
  dW[i] = (float)s;
}

extern "C" int sa_xv_wgrad_reduce(const float* part, int nsplit, int K, int Cout, int Cin, float* dW,
                                  void* stream) {
  if (!part || !dW || nsplit <= 0 || K <= 0 || Cout <= 0 || Cin <= 0) return -22;
  const size_t n = (size_t)K * Cout * Cin;
  hipLaunchKernelGGL(sa_xv_wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), part, nsplit, K, Cout, Cin, dW);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

// ---------------------------------------------------------------------------------
// train-mode data gradient: sa_tdnn_bwd_kernel with the pre-activation gradient dpre [B][T][Cy]
// (BatchNorm train backward and LeakyReLU already applied by sa_xv_colsums) staged as it is.
// dxe [B][T + 2*pad][Cin] on the extended range; sa_tdnn_fold applies the reflect adjoint.
// wp: the data-gradient image of sa_tdnn_bwd_input.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void sa_xv_tdnn_dgrad_kernel(const float* __restrict__ dpre,
                                                                   const bf16x8* __restrict__ wp,
                                                                   float* __restrict__ dxe, int T, int Cy,
                                                                   int Cred, int Cin, int Npad, int K, int dil) {
  constexpr int PITCH = SA_XT_CK + 8, ROWS = SA_XT_BM + SA_XT_HALO, PLANE = ROWS * PITCH;
  __shared__ __attribute__((aligned(16))) bf16_t As[2 * PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int t0 = blockIdx.x * SA_XT_BM, n0 = blockIdx.y * SA_XT_BN, b = blockIdx.z;
  const int pad = dil * (K - 1) / 2, nrows = SA_XT_BM + 2 * pad, Te = T + 2 * pad;
  const int KSTEPS = Cred / 16, NT = Npad / 32;
  const size_t lo_off = (size_t)K * KSTEPS * NT * 64;
  f32x16 acc[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0.0f;
  const float* gb = dpre + (size_t)b * T * Cy;
  for (int c0 = 0; c0 < Cred; c0 += SA_XT_CK) {
    const int ck = Cred - c0 < SA_XT_CK ? Cred - c0 : SA_XT_CK, chunks = ck / 4;
    for (int e = tid; e < nrows * chunks; e += 256) {
      const int r = e / chunks, c = e % chunks, ch = c0 + c * 4;
      const int tt = t0 + r - 2 * pad;
      float f[4] = {0.f, 0.f, 0.f, 0.f};
      if (tt >= 0 && tt < T && ch < Cy) {
        const float4 g = *reinterpret_cast<const float4*>(gb + (size_t)tt * Cy + ch);
        f[0] = g.x; f[1] = g.y; f[2] = g.z; f[3] = g.w;
      }
      uint2 hi, lo;
      sa_split4(f, hi, lo);
      *reinterpret_cast<uint2*>(As + r * PITCH + c * 4) = hi;
      *reinterpret_cast<uint2*>(As + PLANE + r * PITCH + c * 4) = lo;
    }
    __syncthreads();
    const int ksteps = ck / 16;
    for (int k = 0; k < K; ++k) {
      for (int ks = 0; ks < ksteps; ++ks) {
        const bf16x8* wt = wp + (((size_t)(K - 1 - k) * KSTEPS + c0 / 16 + ks) * NT + n0 / 32 + wn * 2) * 64 + lane;
        bf16x8 bh[2], bl[2], ah[2], al[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) { bh[nt] = wt[nt * 64]; bl[nt] = wt[lo_off + nt * 64]; }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          const bf16_t* ap = As + (wm * 64 + mt * 32 + (lane & 31) + k * dil) * PITCH + ks * 16 + 8 * (lane >> 5);
          ah[mt] = *reinterpret_cast<const bf16x8*>(ap);
          al[mt] = *reinterpret_cast<const bf16x8*>(ap + PLANE);
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) {
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mt], bh[nt], acc[mt][nt], 0, 0, 0);
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bl[nt], acc[mt][nt], 0, 0, 0);
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bh[nt], acc[mt][nt], 0, 0, 0);
          }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int n = n0 + (wn * 2 + nt) * 32 + (lane & 31);
    if (n < Cin) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int t = t0 + wm * 64 + mt * 32 + sa_acc_row(i, lane);
          if (t < Te) dxe[((size_t)b * Te + t) * Cin + n] = acc[mt][nt][i];
        }
    }
  }
}

extern "C" int sa_xv_tdnn_dgrad(const float* dpre, const void* wp, float* dxe, int B, int T, int Cy, int Cred,
                                int Cin, int Npad, int K, int dil, void* stream) {
  if (!dpre || !wp || !dxe || B <= 0 || T <= 0 || Cy <= 0 || Cin <= 0 || !sa_xt_reflect_ok(T, K, dil) ||
      Cred % 16 || Cred < Cy || Cy % 4 || Npad % SA_XT_BN || Npad < Cin)
    return -22;
  const int Te = T + dil * (K - 1);
  dim3 grid(sa_div_up(Te, SA_XT_BM), Npad / SA_XT_BN, B);
  hipLaunchKernelGGL(sa_xv_tdnn_dgrad_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), dpre,
                     reinterpret_cast<const bf16x8*>(wp), dxe, T, Cy, Cred, Cin, Npad, K, dil);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

// ---------------------------------------------------------------------------------
// statistics pooling of y = s*z + t (BatchNorm train affine of the last block) from the pooled
// statistics of z (pz = sa_time_pool(z) without noise: mean_z, std_z + eps):
//   mean_y = s*mean_z + t (+ eps*((1-9)*noise + 9)),   std_y + eps = |s|*std_z + eps
// backward: d mean_z-part = g_mean, d std-part = sign(s)*g_std, which sa_time_pool_bwd(z, pz) turns
// into d loss / d y (the (y - mean_y)/std_y of its formula equals sign(s)*(z - mean_z)/std_z).
// ---------------------------------------------------------------------------------
__global__ void sa_xv_pool_affine_kernel(const float* __restrict__ pz, const float* __restrict__ s,
                                         const float* __restrict__ t, const float* __restrict__ noise, int B,
                                         int C, float eps, float* __restrict__ pooled, float* __restrict__ gz,
                                         const float* __restrict__ g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i % C;
  const size_t m = (size_t)b * 2 * C + c, d = m + C;
  if (g) {                                            // backward
    gz[m] = g[m];
    gz[d] = s[c] < 0.0f ? -g[d] : g[d];
    return;
  }
  float mo = fmaf(s[c], pz[m], t[c]);
  if (noise) mo += eps * ((1.0f - 9.0f) * noise[i] + 9.0f);
  pooled[m] = mo;
  pooled[d] = fabsf(s[c]) * (pz[d] - eps) + eps;
}

extern "C" int sa_xv_pool_affine(const float* pz, const float* s, const float* t, const float* noise, int B,
                                 int C, float eps, float* pooled, void* stream) {
  if (!pz || !s || !t || !pooled || B <= 0 || C <= 0) return -22;
  hipLaunchKernelGGL(sa_xv_pool_affine_kernel, dim3(sa_div_up(B * C, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), pz, s, t, noise, B, C, eps, pooled, nullptr, nullptr);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

extern "C" int sa_xv_pool_affine_bwd(const float* g, const float* s, int B, int C, float* gz, void* stream) {
  if (!g || !s || !gz || B <= 0 || C <= 0) return -22;
  hipLaunchKernelGGL(sa_xv_pool_affine_kernel, dim3(sa_div_up(B * C, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), nullptr, s, nullptr, nullptr, B, C, 0.0f, nullptr, gz, g);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
