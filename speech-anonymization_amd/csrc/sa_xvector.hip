// x-vector gender classifier (speechbrain Xvector + Classifier, models/external_gender_classifiers.py:
// 24-183): the frozen eval-mode network (evaluator_inference.yaml:34-41, and inside the training
// graph of models/EndToEnd.py:57-61,81, where only d loss / d features is needed) and the TRAIN mode
// of gender_classifier_train.py (NLL, BatchNorm on batch statistics).  Five TDNN blocks
//   eval :  y = bn_s * LeakyReLU(conv_same_reflect(x) + bias) + bn_t      (running statistics)
//   train:  z = LeakyReLU(conv_same_reflect(x) + bias),  y = BN_train(z) = s*z + t
// with activations [B][T][C] (fp32), split-bf16 MFMA operands on both sides, fp32 accumulation and
// fp64 statistics finalisers (sa_sum_partials / sa_fin_bn_fwd / sa_fin_norm_bwd / sa_fin_bias).
// Nothing here uses float atomics: every reduction is written as fixed-order partials and added in
// a fixed order, so a step gives the same bits on every run.
//   sa_tdnn_fwd            eval block, optionally with the LeakyReLU branch mask for the backward
//   sa_tdnn_bwd_input      d x (extended range) of a frozen eval block from d y and that mask
//   sa_xv_tdnn_fwd_train   z and per-(utterance, 128-frame tile) partials of sum z, sum z^2; the
//                          previous block's BatchNorm affine is applied to the input while staging
//   sa_xv_tdnn_dgrad       d x (extended range) = sum_k W_k^T dpre
//   sa_tdnn_fold           the reflect adjoint: extended range -> d x
//   sa_xv_colsums          per-channel fp64 partials over row chunks of a [M][N] matrix (batch
//                          statistics, BatchNorm backward sums) and, with the folded coefficients,
//                          the pre-activation gradient dpre = leak'(z) * (c1*dy + c2*z + c3)
//   sa_xv_tdnn_wgrad       dW_k = dpre^T x_k over the B*T rows, split across workgroups
//   sa_xv_wgrad_reduce     the split partials added in split order, into the torch [Cout][Cin][K] layout
//   sa_time_pool(_bwd)     statistics pooling over time with relative lengths
//   sa_xv_pool_affine(_bwd) statistics pooling of y = s*z + t from the pooled statistics of z
//   sa_leaky_affine(_bwd)  LeakyReLU -> per-channel affine on the small [B][C] head activations
#include "sa_common.h"
#include "../../include/sa_hip.h"

#define SA_XT_BM 128                      // frames per workgroup (forward / data gradient)
#define SA_XT_BN 128                      // output channels per workgroup
#define SA_XT_CK 64                       // reduction channels per LDS chunk
#define SA_XT_HALO 8                      // >= dil*(K-1) for the x-vector layers (k5 d1, k3 d2, k3 d3)
#define SA_XT_RK 32                       // rows per LDS stage of the weight gradient

static inline int sa_xt_reflect_ok(int T, int K, int dil) {
  return K >= 1 && (K & 1) && dil >= 1 && dil * (K - 1) / 2 < T && dil * (K - 1) <= SA_XT_HALO;
}

// ---------------------------------------------------------------------------------
// The TDNN GEMM tile, shared by the four kernels below.  A TDNN block is a Conv1d with "same"
// reflect padding and dilation on [B][T][C] activations:
//   forward        out[t][co] = sum_{k,ci} x[refl(t + k*dil - pad)][ci] * w[co][ci][k]
//   data gradient  d xe[p][ci] = sum_{k,co} d z[p + pad - k*dil][co] * w[co][ci][k]   on the EXTENDED
//                  range p in [-pad, T + pad), d z zero outside [0, T); sa_tdnn_fold then applies
//                  the adjoint of the reflect padding:
//                  d x[j] = d xe[j] + d xe[-j] (1 <= j <= pad) + d xe[2(T-1) - j] (T-1-pad <= j <= T-2)
// Tiled GEMM on the bf16 MFMA with split (hi/lo) operands, like the conv kernels: one 4-wave
// workgroup = 128 rows x 128 produced channels of one utterance; the reduction channels go through
// LDS in chunks of <= 64 (rows + tap halo staged and split once per chunk, every tap is a row
// offset into the staged tile), weights come as the fragment-major image of sa_pack_weights
// (SA_BF16X3, N padded to a multiple of 128) straight from L2.  Three compile-time policies:
//   Stage  which source row LDS row r holds, what is staged outside the utterance (reflection or
//          zero) and the transform of the four loaded floats:  stage.load(t0 + r, pad, ch, f)
//   Dir    the direction: tap order in the weight image and the number of output rows
//          (SaXtForward: k, T;  SaXtDataGrad: K - 1 - k, T + 2*pad); the reduction width Cred is
//          the block's input channels forward, its padded output channels in the data gradient
//   Epi    the epilogue: begin(col, n) once per owned output column, elem(col, t, n, acc) per
//          accumulator element with t < rows, column_end / tile_end for a reduction through LDS
// The k-loop is the same code for all four: three MFMAs per (mt, nt) in the order al*bh, ah*bl, ah*bh.
// ---------------------------------------------------------------------------------
struct SaXtForward {
  static constexpr bool kReverseTaps = false;
  static __device__ __forceinline__ int rows(int T, int /*pad*/) { return T; }
};
struct SaXtDataGrad {
  static constexpr bool kReverseTaps = true;
  static __device__ __forceinline__ int rows(int T, int pad) { return T + 2 * pad; }
};

template <class Dir, class Stage, class Epi>
__device__ __forceinline__ void sa_xt_tile(const Stage stage, const bf16x8* __restrict__ wp, int T, int Cred,
                                           int Npad, int Nout, int K, int dil, Epi epi) {
  constexpr int PITCH = SA_XT_CK + 8, ROWS = SA_XT_BM + SA_XT_HALO, PLANE = ROWS * PITCH;
  __shared__ __attribute__((aligned(16))) bf16_t As[2 * PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int t0 = blockIdx.x * SA_XT_BM, n0 = blockIdx.y * SA_XT_BN;
  const int pad = dil * (K - 1) / 2, nrows = SA_XT_BM + 2 * pad, rows = Dir::rows(T, pad);
  const int KSTEPS = Cred / 16, NT = Npad / 32;
  const size_t lo_off = (size_t)K * KSTEPS * NT * 64;            // fragments per weight plane
  f32x16 acc[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0.0f;
  for (int c0 = 0; c0 < Cred; c0 += SA_XT_CK) {
    const int ck = Cred - c0 < SA_XT_CK ? Cred - c0 : SA_XT_CK, chunks = ck / 4;
    // ---- stage BM + 2*pad rows of this channel chunk, split hi / lo ----
    for (int e = tid; e < nrows * chunks; e += 256) {
      const int r = e / chunks, c = e % chunks;
      float f[4] = {0.f, 0.f, 0.f, 0.f};
      stage.load(t0 + r, pad, c0 + c * 4, f);
      uint2 hi, lo;
      sa_split4(f, hi, lo);
      *reinterpret_cast<uint2*>(As + r * PITCH + c * 4) = hi;
      *reinterpret_cast<uint2*>(As + PLANE + r * PITCH + c * 4) = lo;
    }
    __syncthreads();
    const int ksteps = ck / 16;
    for (int k = 0; k < K; ++k) {
      const int kw = Dir::kReverseTaps ? K - 1 - k : k;
      for (int ks = 0; ks < ksteps; ++ks) {
        const bf16x8* wt = wp + (((size_t)kw * KSTEPS + c0 / 16 + ks) * NT + n0 / 32 + wn * 2) * 64 + lane;
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
  float* red = reinterpret_cast<float*>(As);           // free after the last barrier
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int nl = (wn * 2 + nt) * 32 + (lane & 31), n = n0 + nl;
    typename Epi::Col col = {};
    if (n < Nout) {
      epi.begin(col, n);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int t = t0 + wm * 64 + mt * 32 + sa_acc_row(i, lane);
          if (t < rows) epi.elem(col, t, n, acc[mt][nt][i]);
        }
    }
    epi.column_end(col, red, wm, nl, lane);
  }
  epi.tile_end(red, tid, n0);
}

// ---- staging policies.  Xf(off, ch, f): transform of the four floats loaded from element offset
// `off` (= row*C + ch) of the utterance ----
struct SaXtNoXf {
  __device__ __forceinline__ void operator()(size_t, int, float*) const {}
};
// forward: LDS row r <- source row t0 + r - pad, reflected at the utterance ends (no edge repeat)
template <class Xf>
struct SaXtStageReflect {
  const float* __restrict__ x;            // this utterance, [T][C]
  int T, C;
  Xf xf;
  __device__ __forceinline__ void load(int t0r, int pad, int ch, float* f) const {
    int tt = t0r - pad;
    if (tt < 0) tt = -tt;
    if (tt >= T) tt = 2 * (T - 1) - tt;
    if (tt >= 0 && tt < T) {
      const size_t off = (size_t)tt * C + ch;
      const float4 v = *reinterpret_cast<const float4*>(x + off);
      f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
      xf(off, ch, f);
    }
  }
};
// data gradient: extended output row t0 + r uses d z[t0 + r - 2*pad + k'*dil]; zero outside the
// utterance and in the reduction channels padded beyond C
template <class Xf>
struct SaXtStageZero {
  const float* __restrict__ x;
  int T, C;
  Xf xf;
  __device__ __forceinline__ void load(int t0r, int pad, int ch, float* f) const {
    const int tt = t0r - 2 * pad;
    if (tt >= 0 && tt < T && ch < C) {
      const size_t off = (size_t)tt * C + ch;
      const float4 v = *reinterpret_cast<const float4*>(x + off);
      f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
      xf(off, ch, f);
    }
  }
};
// x' = s*x + t per input channel: the previous block's BatchNorm(train); none when s == null
struct SaXtAffineXf {
  const float* __restrict__ s;
  const float* __restrict__ t;
  __device__ __forceinline__ void operator()(size_t, int ch, float* f) const {
    if (s) {
#pragma unroll
      for (int j = 0; j < 4; ++j) f[j] = fmaf(s[ch + j], f[j], t[ch + j]);
    }
  }
};
// d z = d y * bn_s * (z > 0 ? 1 : slope): BatchNorm(eval) and LeakyReLU backward, z > 0 from the
// branch mask the forward wrote (recovering the sign from the stored y = s*leaky(z) + t cancels
// for small z)
struct SaXtFrozenBwdXf {
  const unsigned char* __restrict__ mask; // this utterance, [T][C]
  const float* __restrict__ bn_s;
  float slope;
  __device__ __forceinline__ void operator()(size_t off, int ch, float* f) const {
    const uchar4 m4 = *reinterpret_cast<const uchar4*>(mask + off);
    const unsigned char mm[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = f[j] * (bn_s ? bn_s[ch + j] : 1.0f) * (mm[j] ? 1.0f : slope);
  }
};

// ---- epilogues ----
// bias -> LeakyReLU (branch mask for the backward on request) -> BatchNorm(eval) affine -> store
struct SaXtEpiEval {
  const float* __restrict__ bias;
  const float* __restrict__ bn_s;
  const float* __restrict__ bn_t;
  float* __restrict__ y;                  // this utterance, [T][Cout]
  unsigned char* __restrict__ mask;
  int Cout;
  float slope;
  struct Col { float bb, sc, sh; };
  __device__ __forceinline__ void begin(Col& c, int n) const {
    c.bb = bias ? bias[n] : 0.0f; c.sc = bn_s ? bn_s[n] : 1.0f; c.sh = bn_t ? bn_t[n] : 0.0f;
  }
  __device__ __forceinline__ void elem(Col& c, int t, int n, float a) const {
    float v = a + c.bb;
    if (mask) mask[(size_t)t * Cout + n] = v > 0.0f;
    v = v > 0.0f ? v : v * slope;
    y[(size_t)t * Cout + n] = fmaf(v, c.sc, c.sh);
  }
  __device__ __forceinline__ void column_end(Col&, float*, int, int, int) const {}
  __device__ __forceinline__ void tile_end(float*, int, int) const {}
};
// z = leaky(acc + bias) stored, and part[n][0..1] = (sum z, sum z^2) over the tile's valid frames
// (fp32, fixed order: the two half-waves, then the two waves that share the columns)
struct SaXtEpiTrain {
  const float* __restrict__ bias;
  float* __restrict__ z;                  // this utterance, [T][Cout]
  float* __restrict__ part;               // this (utterance, tile), [Cout][2]
  int Cout;
  float slope;
  struct Col { float bb, s, q; };
  __device__ __forceinline__ void begin(Col& c, int n) const { c.bb = bias ? bias[n] : 0.0f; }
  __device__ __forceinline__ void elem(Col& c, int t, int n, float a) const {
    float v = a + c.bb;
    v = v > 0.0f ? v : v * slope;
    z[(size_t)t * Cout + n] = v;
    c.s += v; c.q = fmaf(v, v, c.q);
  }
  // red: [2 waves along frames][128 columns][2]
  __device__ __forceinline__ void column_end(Col& c, float* red, int wm, int nl, int lane) const {
    c.s += __shfl_xor(c.s, 32, 64);
    c.q += __shfl_xor(c.q, 32, 64);
    if (lane < 32) { red[(wm * 128 + nl) * 2] = c.s; red[(wm * 128 + nl) * 2 + 1] = c.q; }
  }
  __device__ __forceinline__ void tile_end(float* red, int tid, int n0) const {
    __syncthreads();
    if (tid < SA_XT_BN && n0 + tid < Cout) {
      float* o = part + (size_t)(n0 + tid) * 2;
      o[0] = red[tid * 2] + red[(128 + tid) * 2];
      o[1] = red[tid * 2 + 1] + red[(128 + tid) * 2 + 1];
    }
  }
};
// plain store on the extended range
struct SaXtEpiStore {
  float* __restrict__ dxe;                // this utterance, [T + 2*pad][Cin]
  int Cin;
  struct Col {};
  __device__ __forceinline__ void begin(Col&, int) const {}
  __device__ __forceinline__ void elem(Col&, int t, int n, float a) const { dxe[(size_t)t * Cin + n] = a; }
  __device__ __forceinline__ void column_end(Col&, float*, int, int, int) const {}
  __device__ __forceinline__ void tile_end(float*, int, int) const {}
};

// ---------------------------------------------------------------------------------
// eval forward: speechbrain Conv1d ("same" reflect padding, dilation) -> LeakyReLU ->
// BatchNorm1d(eval), the block of models/external_gender_classifiers.py:71-87
//   y[b][t][co] = bn_s[co] * leaky( bias[co] + sum_{k,ci} x[b][refl(t + k*dil - pad)][ci] * w[co][ci][k] ) + bn_t[co]
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void sa_tdnn_fwd_kernel(const float* __restrict__ x,
                                                             const bf16x8* __restrict__ wp,
                                                             const float* __restrict__ bias,
                                                             const float* __restrict__ bn_s,
                                                             const float* __restrict__ bn_t,
                                                             float* __restrict__ y, int T, int Cin,
                                                             int Cout, int Npad, int K, int dil,
                                                             float slope, unsigned char* __restrict__ mask) {
  const size_t b = blockIdx.z;
  const SaXtStageReflect<SaXtNoXf> stage = {x + b * T * Cin, T, Cin, {}};
  const SaXtEpiEval epi = {bias, bn_s, bn_t, y + b * T * Cout, mask ? mask + b * T * Cout : nullptr, Cout, slope};
  sa_xt_tile<SaXtForward>(stage, wp, T, Cin, Npad, Cout, K, dil, epi);
}

// wp: sa_pack_weights(SA_BF16X3, w padded to Npad output channels, ntaps = K, K = Cin, N = Npad,
// sk = K, sn = Cin*K, st = 1); Npad % 128 == 0, Cin % 16 == 0.
extern "C" int sa_tdnn_fwd(const float* x, const void* wp, const float* bias, const float* bn_s,
                           const float* bn_t, float* y, int B, int T, int Cin, int Cout, int Npad, int K,
                           int dil, float slope, unsigned char* mask, void* stream) {
  if (!x || !wp || !y || B <= 0 || T <= 0 || Cin <= 0 || Cout <= 0 || !sa_xt_reflect_ok(T, K, dil) ||
      Cin % 16 || Npad % SA_XT_BN || Npad < Cout)
    return -22;
  dim3 grid(sa_div_up(T, SA_XT_BM), Npad / SA_XT_BN, B);
  hipLaunchKernelGGL(sa_tdnn_fwd_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x,
                     reinterpret_cast<const bf16x8*>(wp), bias, bn_s, bn_t, y, T, Cin, Cout, Npad, K, dil,
                     slope, mask);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

// ---------------------------------------------------------------------------------
// Input gradient of a (frozen, eval-mode) TDNN block  y = BN_eval(LeakyReLU(conv_same_reflect(x)))
// (models/EndToEnd.py:57-61,81: the pretrained x-vector classifier sits in the training graph
// with requires_grad off, so only d loss / d x is needed).  d z is formed from d y, bn_s and the
// forward's mask while staging; d xe on the extended range goes to sa_tdnn_fold.
// wp: sa_pack_weights(SA_BF16X3, ...) image of the Conv1d weight as a DATA-GRADIENT operand
// (reduction = the block's output channels, zero-padded to Cred % 16 == 0; produced = its input
// channels, zero-padded to Npad % 128 == 0): ntaps = K, K = Cred, N = Npad, sk = Cin_w*K, sn = K, st = 1.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void sa_tdnn_bwd_kernel(const float* __restrict__ dy,
                                                              const unsigned char* __restrict__ mask,
                                                              const float* __restrict__ bn_s,
                                                              const bf16x8* __restrict__ wp,
                                                              float* __restrict__ dxe, int T, int Cy,
                                                              int Cred, int Cin, int Npad, int K, int dil,
                                                              float slope) {
  const size_t b = blockIdx.z;
  const int Te = T + dil * (K - 1);
  const SaXtStageZero<SaXtFrozenBwdXf> stage = {dy + b * T * Cy, T, Cy, {mask + b * T * Cy, bn_s, slope}};
  const SaXtEpiStore epi = {dxe + b * Te * Cin, Cin};
  sa_xt_tile<SaXtDataGrad>(stage, wp, T, Cred, Npad, Cin, K, dil, epi);
}

// dxe: [B][T + 2*pad][Cin] (pad = dil*(K-1)/2), caller-allocated; feed it to sa_tdnn_fold.
extern "C" int sa_tdnn_bwd_input(const float* dy, const unsigned char* mask, const float* bn_s,
                                 const void* wp, float* dxe, int B, int T, int Cy, int Cred, int Cin,
                                 int Npad, int K, int dil, float slope, void* stream) {
  if (!dy || !mask || !wp || !dxe || B <= 0 || T <= 0 || Cy <= 0 || Cin <= 0 || !sa_xt_reflect_ok(T, K, dil) ||
      Cred % 16 || Cred < Cy || Cy % 4 || Npad % SA_XT_BN || Npad < Cin)
    return -22;
  const int Te = T + dil * (K - 1);
  dim3 grid(sa_div_up(Te, SA_XT_BM), Npad / SA_XT_BN, B);
  hipLaunchKernelGGL(sa_tdnn_bwd_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), dy, mask,
                     bn_s, reinterpret_cast<const bf16x8*>(wp), dxe, T, Cy, Cred, Cin, Npad, K, dil,
                     slope);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

// ---------------------------------------------------------------------------------
// train-mode forward.  Prologue: x = s_in*x + t_in per input channel (the previous block's
// BatchNorm; none for block 0).  Epilogue: z = leaky(acc + bias) stored, and
// part[b*ntile + tile][n][0..1] = (sum z, sum z^2) over the tile's valid frames.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void sa_xv_tdnn_fwd_train_kernel(
    const float* __restrict__ x, const float* __restrict__ s_in, const float* __restrict__ t_in,
    const bf16x8* __restrict__ wp, const float* __restrict__ bias, float* __restrict__ z,
    float* __restrict__ part, int T, int Cin, int Cout, int Npad, int K, int dil, float slope) {
  const size_t b = blockIdx.z;
  const SaXtStageReflect<SaXtAffineXf> stage = {x + b * T * Cin, T, Cin, {s_in, t_in}};
  const SaXtEpiTrain epi = {bias, z + b * T * Cout, part + (b * gridDim.x + blockIdx.x) * Cout * 2, Cout, slope};
  sa_xt_tile<SaXtForward>(stage, wp, T, Cin, Npad, Cout, K, dil, epi);
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
// train-mode data gradient: the pre-activation gradient dpre [B][T][Cy] (BatchNorm train backward
// and LeakyReLU already applied by sa_xv_colsums) staged as it is.
// dxe [B][T + 2*pad][Cin] on the extended range; sa_tdnn_fold applies the reflect adjoint.
// wp: the data-gradient image of sa_tdnn_bwd_input.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void sa_xv_tdnn_dgrad_kernel(const float* __restrict__ dpre,
                                                                   const bf16x8* __restrict__ wp,
                                                                   float* __restrict__ dxe, int T, int Cy,
                                                                   int Cred, int Cin, int Npad, int K, int dil) {
  const size_t b = blockIdx.z;
  const int Te = T + dil * (K - 1);
  const SaXtStageZero<SaXtNoXf> stage = {dpre + b * T * Cy, T, Cy, {}};
  const SaXtEpiStore epi = {dxe + b * Te * Cin, Cin};
  sa_xt_tile<SaXtDataGrad>(stage, wp, T, Cred, Npad, Cin, K, dil, epi);
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

// adjoint of the reflect padding: dx[j] = dxe[j + pad] + dxe[pad - j] (1 <= j <= pad)
//                                       + dxe[2(T-1) - j + pad] (T-1-pad <= j <= T-2)
__global__ void sa_tdnn_fold_kernel(const float* __restrict__ dxe, float* __restrict__ dx, int T, int C,
                                    int pad, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const size_t bt = i / C;
  const int j = (int)(bt % T);
  const size_t b = bt / T;
  const float* e = dxe + (b * (size_t)(T + 2 * pad)) * C + c;
  float v = e[(size_t)(j + pad) * C];
  if (j >= 1 && j <= pad) v += e[(size_t)(pad - j) * C];
  if (j >= T - 1 - pad && j <= T - 2) v += e[(size_t)(2 * (T - 1) - j + pad) * C];
  dx[i] = v;
}

extern "C" int sa_tdnn_fold(const float* dxe, float* dx, int B, int T, int C, int pad, void* stream) {
  if (!dxe || !dx || B <= 0 || T <= 0 || C <= 0 || pad < 0 || pad >= T) return -22;
  const size_t total = (size_t)B * T * C;
  hipLaunchKernelGGL(sa_tdnn_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), dxe, dx, T, C, pad, total);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

// backward of sa_time_pool (statistics over the first n = round(len*T) frames):
//   dx[t][c] = g_mean[c]/n + g_std[c] * (x[t][c] - mean[c]) / ((n-1) * std[c])   for t < n, else 0
// pooled = the forward output [B][2C] WITHOUT the noise offset on the mean half (mean, std + eps).
__global__ void sa_time_pool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ lens,
                                        const float* __restrict__ g, const float* __restrict__ pooled,
                                        int T, int C, float eps, float* __restrict__ dx, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const size_t bt = i / C;
  const int t = (int)(bt % T);
  const size_t b = bt / T;
  int n = lens ? (int)rintf(lens[b] * (float)T) : T;
  if (n > T) n = T;
  float v = 0.0f;
  if (t < n) {
    const float m = pooled[b * 2 * C + c], sd = pooled[b * 2 * C + C + c] - eps;
    v = g[b * 2 * C + c] / (float)n;
    if (n > 1 && sd > 0.0f) v += g[b * 2 * C + C + c] * (x[i] - m) / ((float)(n - 1) * sd);
  }
  dx[i] = v;
}

extern "C" int sa_time_pool_bwd(const float* x, const float* lens, const float* g, const float* pooled,
                                int B, int T, int C, float eps, float* dx, void* stream) {
  if (!x || !g || !pooled || !dx || B <= 0 || T <= 0 || C <= 0) return -22;
  const size_t total = (size_t)B * T * C;
  hipLaunchKernelGGL(sa_time_pool_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, lens, g, pooled, T, C, eps, dx, total);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

// backward of sa_leaky_affine: dx = dy * s[c] * (x > 0 ? 1 : slope)
__global__ void sa_leaky_affine_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                           const float* __restrict__ s, float slope, int M, int C, float* dx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * C) return;
  dx[i] = dy[i] * (s ? s[i % C] : 1.0f) * (x[i] > 0.0f ? 1.0f : slope);
}

extern "C" int sa_leaky_affine_bwd(const float* dy, const float* x, const float* s, float slope, int M, int C,
                                   float* dx, void* stream) {
  if (!dy || !x || !dx) return -22;
  hipLaunchKernelGGL(sa_leaky_affine_bwd_kernel, dim3(sa_div_up(M * C, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), dy, x, s, slope, M, C, dx);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

// speechbrain StatisticsPooling over time with relative lengths: mean and unbiased std (+eps) of
// the first round(len*T) frames per (utterance, channel); out [B][2C] = (mean (+noise), std).
__global__ void sa_time_pool_kernel(const float* __restrict__ x, const float* __restrict__ lens,
                                    const float* __restrict__ noise, int T, int C, float eps,
                                    float* __restrict__ out) {
  const int b = blockIdx.y, c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  int n = lens ? (int)rintf(lens[b] * (float)T) : T;
  if (n > T) n = T;
  double s = 0.0, q = 0.0;
  for (int t = 0; t < n; ++t) {
    const double v = x[((size_t)b * T + t) * C + c];
    s += v; q += v * v;
  }
  const double m = s / n;
  double var = n > 1 ? (q - s * m) / (n - 1) : 0.0;
  if (var < 0.0) var = 0.0;
  float mo = (float)m;
  if (noise) mo += eps * ((1.0f - 9.0f) * noise[(size_t)b * C + c] + 9.0f);
  out[(size_t)b * 2 * C + c] = mo;
  out[(size_t)b * 2 * C + C + c] = (float)sqrt(var) + eps;
}

extern "C" int sa_time_pool(const float* x, const float* lens, const float* noise, int B, int T, int C,
                            float eps, float* out, void* stream) {
  if (!x || !out || B <= 0 || T <= 0 || C <= 0) return -22;
  hipLaunchKernelGGL(sa_time_pool_kernel, dim3(sa_div_up(C, 128), B), dim3(128), 0,
                     reinterpret_cast<hipStream_t>(stream), x, lens, noise, T, C, eps, out);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

// y = x > 0 ? x : slope*x, then *s[c] + t[c]  (LeakyReLU -> BatchNorm(eval) on a small [M][C])
__global__ void sa_leaky_affine_kernel(const float* __restrict__ x, const float* __restrict__ s,
                                       const float* __restrict__ t, float slope, int M, int C, float* y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * C) return;
  float v = x[i];
  v = v > 0.0f ? v : v * slope;
  y[i] = s ? fmaf(v, s[i % C], t[i % C]) : v;
}

extern "C" int sa_leaky_affine(const float* x, const float* s, const float* t, float slope, int M, int C,
                               float* y, void* stream) {
  if (!x || !y) return -22;
  hipLaunchKernelGGL(sa_leaky_affine_kernel, dim3(sa_div_up(M * C, 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), x, s, t, slope, M, C, y);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

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

