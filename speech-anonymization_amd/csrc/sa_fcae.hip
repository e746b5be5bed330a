// model_type fcae: the train path of the reference's FullyConnectedAutoencoder
// (models/FullyConnected.py:65-104,118-159) in nine launches, fp32 throughout.
//
//   encoder  Linear(80,60) ReLU Linear(60,40) ReLU Linear(40,20)                      -> z [B][T][20]
//   decoder  Linear(20,40) ReLU Linear(40,60) ReLU Linear(60,80)                      -> recon
//   sex_classifier: GradReverse, reshape(B,20,T) -> BatchNorm1d(20) -> reshape(B,T,20) (a reinterpretation:
//     element (t, j) of an utterance belongs to channel (20 t + j) / T), initial = Linear(20,40) ReLU
//     Linear(40,40) ReLU, StatisticsPooling over time, classify = Linear(80,40) BatchNorm ReLU Linear(40,40)
//     ReLU Linear(40,20) BatchNorm Linear(20,2), log_softmax.
//
// Every per-frame layer is a [frames x K] x [K x N] product with K, N <= 80.  A workgroup owns a tile of
// FC_TM = 64 frames of one utterance (tiles never cross utterances, so the pooling sums are per tile),
// keeps the tile's activations in LDS from the first layer to the last and stages one weight matrix at a
// time beside them.  The products are fp32 FMA loops on 4 x J register tiles (v_fmac_f32; the layers are
// too narrow to fill a 32x32 MFMA tile and the step is bound by its launch count).
// The hidden activations are STORED by the forward (300 floats per frame) and read back by the backward.
//
// forward : sa_fc_enc_fwd -> sa_fc_bn_fin -> sa_fc_mid_fwd -> sa_fc_head_fwd
// inference (reconstruction only): sa_fc_recon_fwd, one launch
// backward: sa_fc_head_bwd -> sa_fc_mid_bwd -> sa_fc_bn_bwd_fin -> sa_fc_enc_bwd -> sa_fc_wreduce
//
// Statistics (BatchNorm channel sums, pooling sums) and the weight-gradient splits are accumulated per
// workgroup, written as partials and added in fp64 in a fixed order: no atomics, bit-reproducible.
#include "sa_common.h"

#define FC_TM 64
#define FC_NT 256
#define FC_MAXG 256
#define FC_MAXB 64
#define FC_NPARAM 18780          /* 18400 weights + 380 biases of the eight per-frame Linears */
#define FC_NHEAD 5862            /* the twelve head gradients */

namespace {

// layer l of FcW: 0..2 encoder.0/2/4, 3..5 decoder.0/2/4, 6..7 sex_classifier.initial.0/2
struct FcW { const float* w[8]; const float* b[8]; };
// offsets of layer l's weight / bias gradient in a [FC_NPARAM] record (all weights, then all biases)
constexpr int fc_woff(int l) {
  const int n[8] = {4800, 2400, 800, 800, 2400, 4800, 800, 1600};
  int o = 0;
  for (int i = 0; i < l; ++i) o += n[i];
  return o;
}
constexpr int fc_boff(int l) {
  const int n[8] = {60, 40, 20, 40, 60, 80, 40, 40};
  int o = 18400;
  for (int i = 0; i < l; ++i) o += n[i];
  return o;
}
template <int L> constexpr int WOFF = fc_woff(L);
template <int L> constexpr int BOFF = fc_boff(L);
constexpr int WL_FLOATS = 5040;                                  // largest staged matrix: 60 rows of pitch 84

// LDS pitch of a staged matrix with K floats per row: an odd number of 16-byte slots, so that the
// ds_read_b128 of 16 consecutive rows is conflict-free
template <int K> __host__ __device__ constexpr int wpitch() { return ((K / 4) | 1) * 4; }

// W [N][K] (nn.Linear layout) -> LDS rows n
template <int N, int K>
__device__ __forceinline__ void stage_w(float* Wl, const float* W, int tid) {
  constexpr int P = wpitch<K>();
  for (int i = tid; i < N * (K / 4); i += FC_NT) {
    const int n = i / (K / 4), q = i % (K / 4);
    *reinterpret_cast<float4*>(Wl + n * P + 4 * q) = *reinterpret_cast<const float4*>(W + n * K + 4 * q);
  }
}
// W [N][K] -> LDS rows k (the transposed matrix: the operand of the data gradient)
template <int N, int K>
__device__ __forceinline__ void stage_wt(float* Wl, const float* W, int tid) {
  constexpr int P = wpitch<N>();
  for (int i = tid; i < N * K; i += FC_NT) {
    const int n = i / K, k = i % K;
    Wl[k * P + n] = W[i];
  }
}

// rows [0, nvalid) of a tile from global memory (contiguous, 16-byte chunks), zeros behind them
template <int C>
__device__ __forceinline__ void load_tile(float* dst, const float* src, int nvalid, int tid) {
  for (int i = tid; i < FC_TM * (C / 4); i += FC_NT) {
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (i / (C / 4) < nvalid) v = reinterpret_cast<const float4*>(src)[i];
    reinterpret_cast<float4*>(dst)[i] = v;
  }
}

// ep(m, n, sum_k A[m][k] * Wl[n][k]) for the 64 x N outputs of a tile.  A: LDS [64][K]; Wl: LDS [N] rows of
// pitch wpitch<K>.  Thread = 4 rows x J columns (n = ng + 16 j).
template <int K, int N, class EP>
__device__ __forceinline__ void tile_gemm(const float* A, const float* Wl, int tid, EP ep) {
  constexpr int P = wpitch<K>(), J = (N + 15) / 16;
  const int ng = tid & 15, m0 = (tid >> 4) * 4;
  float acc[4][J];
  const float* wp[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int n = ng + 16 * j;
    wp[j] = Wl + (n < N ? n : N - 1) * P;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r][j] = 0.0f;
  }
  const float* ap = A + m0 * K;
#pragma unroll 2
  for (int k = 0; k < K; k += 4) {
    float4 a[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = *reinterpret_cast<const float4*>(ap + r * K + k);
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const float4 w = *reinterpret_cast<const float4*>(wp[j] + k);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[r][j] = fmaf(a[r].x, w.x, acc[r][j]);
        acc[r][j] = fmaf(a[r].y, w.y, acc[r][j]);
        acc[r][j] = fmaf(a[r].z, w.z, acc[r][j]);
        acc[r][j] = fmaf(a[r].w, w.w, acc[r][j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int n = ng + 16 * j;
    if (n < N) {
#pragma unroll
      for (int r = 0; r < 4; ++r) ep(m0 + r, n, acc[r][j]);
    }
  }
}

// weight gradient of a tile: acc += dY^T X, dY LDS [64][N], X LDS [64][K] (rows behind the tile's last
// frame are zero in dY).  The N x K outputs are 4 x 4 blocks; thread tid owns blocks tid, tid + 256, ...
template <int N, int K> struct WgAcc {
  static constexpr int NBLK = (N / 4) * (K / 4), NB = (NBLK + FC_NT - 1) / FC_NT;
  float v[NB][16];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int j = 0; j < 16; ++j) v[i][j] = 0.0f;
  }
  __device__ __forceinline__ void add(const float* dY, const float* X, int tid) {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int blk = tid + i * FC_NT;
      if (blk < NBLK) {
        const float* dp = dY + 4 * (blk / (K / 4));
        const float* xp = X + 4 * (blk % (K / 4));
#pragma unroll 4
        for (int m = 0; m < FC_TM; ++m) {
          const float4 d = *reinterpret_cast<const float4*>(dp + m * N);
          const float4 x = *reinterpret_cast<const float4*>(xp + m * K);
          const float dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            v[i][4 * r + 0] = fmaf(dv[r], x.x, v[i][4 * r + 0]);
            v[i][4 * r + 1] = fmaf(dv[r], x.y, v[i][4 * r + 1]);
            v[i][4 * r + 2] = fmaf(dv[r], x.z, v[i][4 * r + 2]);
            v[i][4 * r + 3] = fmaf(dv[r], x.w, v[i][4 * r + 3]);
          }
        }
      }
    }
  }
  // this workgroup's partial of d W [N][K]
  __device__ __forceinline__ void store(float* dst, int tid) const {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int blk = tid + i * FC_NT;
      if (blk < NBLK) {
        const int n0 = 4 * (blk / (K / 4)), k0 = 4 * (blk % (K / 4));
#pragma unroll
        for (int r = 0; r < 4; ++r)
          *reinterpret_cast<float4*>(dst + (n0 + r) * K + k0) =
              make_float4(v[i][4 * r], v[i][4 * r + 1], v[i][4 * r + 2], v[i][4 * r + 3]);
      }
    }
  }
};

// bias gradient: column sums of dY [64][N] (thread n)
template <int N>
__device__ __forceinline__ void bias_add(float& acc, const float* dY, int tid) {
  if (tid < N) {
    float s = 0.0f;
#pragma unroll 8
    for (int m = 0; m < FC_TM; ++m) s += dY[m * N + tid];
    acc += s;
  }
}

// Sums over the BatchNorm channels a tile touches.  The tile holds the flat elements [20 t0, 20 (t0 + nvalid))
// of its utterance, channel c the flat elements [c T, (c + 1) T).  f(e_local, c, a, b) adds element e_local's
// two terms.  12 strided partial sums per channel (fp64), added in order; thread 2c + comp (< 40) receives
// the result through out(c, comp, value).
template <class F, class OUT>
__device__ __forceinline__ void tile_chan_sums(int T, int t0, int nvalid, int tid, double* red, F f, OUT out) {
  if (tid < 240) {
    const int c = tid / 12, s = tid % 12;
    const int e0 = 20 * t0;
    const int lo = max(c * T, e0), hi = min((c + 1) * T, e0 + 20 * nvalid);
    double a = 0.0, b = 0.0;
    for (int e = lo + s; e < hi; e += 12) f(e - e0, c, a, b);
    red[2 * tid] = a; red[2 * tid + 1] = b;
  }
  __syncthreads();
  if (tid < 40) {
    const int c = tid >> 1, comp = tid & 1;
    double v = 0.0;
    for (int s = 0; s < 12; ++s) v += red[2 * (c * 12 + s) + comp];
    out(c, comp, v);
  }
}

constexpr size_t fc_lds(int act_floats_per_row) {
  return ((size_t)FC_TM * act_floats_per_row + WL_FLOATS) * sizeof(float) + 480 * sizeof(double) + 64 * sizeof(double);
}

// ---------------------------------------------------------------------------------------------------
// forward 1: encoder.  feats -> h1, h2 (post-ReLU), z; per-tile BatchNorm channel sums (sum, sum of squares)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FC_NT) void fc_enc_fwd_kernel(const float* __restrict__ feats, FcW W, float* __restrict__ h1,
                                                           float* __restrict__ h2, float* __restrict__ z,
                                                           double* __restrict__ bnpart, int T) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* red = reinterpret_cast<double*>(smem);                 // [480] + [64]
  float* X = reinterpret_cast<float*>(red + 544);                // [64][80]
  float* H1 = X + FC_TM * 80;                                    // [64][60]
  float* H2 = H1 + FC_TM * 60;                                   // [64][40]
  float* Z = H2 + FC_TM * 40;                                    // [64][20]
  float* Wl = Z + FC_TM * 20;
  const int tid = threadIdx.x, ti = blockIdx.x, b = blockIdx.y, t0 = ti * FC_TM;
  const int nvalid = min(FC_TM, T - t0);
  const size_t f0 = (size_t)b * T + t0;
  load_tile<80>(X, feats + f0 * 80, nvalid, tid);
  stage_w<60, 80>(Wl, W.w[0], tid);
  __syncthreads();
  tile_gemm<80, 60>(X, Wl, tid, [&](int m, int n, float v) {
    v = fmaxf(v + W.b[0][n], 0.0f);
    H1[m * 60 + n] = v;
    if (m < nvalid) h1[(f0 + m) * 60 + n] = v;
  });
  __syncthreads();
  stage_w<40, 60>(Wl, W.w[1], tid);
  __syncthreads();
  tile_gemm<60, 40>(H1, Wl, tid, [&](int m, int n, float v) {
    v = fmaxf(v + W.b[1][n], 0.0f);
    H2[m * 40 + n] = v;
    if (m < nvalid) h2[(f0 + m) * 40 + n] = v;
  });
  __syncthreads();
  stage_w<20, 40>(Wl, W.w[2], tid);
  __syncthreads();
  tile_gemm<40, 20>(H2, Wl, tid, [&](int m, int n, float v) {
    v += W.b[2][n];
    Z[m * 20 + n] = v;
    if (m < nvalid) z[(f0 + m) * 20 + n] = v;
  });
  __syncthreads();
  double* part = bnpart + ((size_t)b * gridDim.x + ti) * 40;
  tile_chan_sums(T, t0, nvalid, tid, red,
                 [&](int e, int, double& a, double& q) { const double v = Z[e]; a += v; q += v * v; },
                 [&](int c, int comp, double v) { part[2 * c + comp] = v; });
}

// ---------------------------------------------------------------------------------------------------
// forward 2: BatchNorm1d(20) finaliser.  train: batch statistics from the tile partials (fp64, fixed order) +
// running statistics (momentum, unbiased variance); eval: the running statistics.  bnf [4][20] = mean, rstd,
// scale, shift
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FC_NT) void fc_bn_fin_kernel(const double* __restrict__ bnpart, int npart,
                                                          const float* gamma, const float* beta, float* run_mean,
                                                          float* run_var, float* bnf, double count, int train,
                                                          float eps, float momentum) {
  __shared__ double red[240];
  const int tid = threadIdx.x;
  if (train && tid < 240) {
    const int v = tid % 40, s = tid / 40;
    double a = 0.0;
    for (int p = s; p < npart; p += 6) a += bnpart[(size_t)p * 40 + v];
    red[tid] = a;
  }
  __syncthreads();
  if (tid < 20) {
    double mu, var;
    if (train) {
      double S = 0.0, Q = 0.0;
      for (int s = 0; s < 6; ++s) { S += red[s * 40 + 2 * tid]; Q += red[s * 40 + 2 * tid + 1]; }
      mu = S / count;
      var = Q / count - mu * mu;
      if (var < 0.0) var = 0.0;
      const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
      run_mean[tid] = (1.0f - momentum) * run_mean[tid] + momentum * (float)mu;
      run_var[tid] = (1.0f - momentum) * run_var[tid] + momentum * (float)unb;
    } else {
      mu = run_mean[tid]; var = run_var[tid];
    }
    const float r = (float)(1.0 / sqrt(var + (double)eps));
    const float sc = gamma[tid] * r;
    bnf[tid] = (float)mu; bnf[20 + tid] = r; bnf[40 + tid] = sc; bnf[60 + tid] = beta[tid] - (float)mu * sc;
  }
}

// ---------------------------------------------------------------------------------------------------
// forward 3: z -> BatchNorm affine by the channel map -> initial (a1, u) + per-tile pooling sums; decoder
// (d1, d2, recon)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FC_NT) void fc_mid_fwd_kernel(const float* __restrict__ z, const float* __restrict__ bnf, FcW W,
                                                           float* __restrict__ a1, float* __restrict__ u,
                                                           float* __restrict__ d1, float* __restrict__ d2,
                                                           float* __restrict__ recon, double* __restrict__ poolpart,
                                                           int T) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* red = reinterpret_cast<double*>(smem);
  float* Z = reinterpret_cast<float*>(red + 544);                // [64][20]
  float* ZN = Z + FC_TM * 20;                                    // [64][20]
  float* A1 = ZN + FC_TM * 20;                                   // [64][40]  a1, later d1
  float* U = A1 + FC_TM * 40;                                    // [64][40]
  float* D2 = U + FC_TM * 40;                                    // [64][60]
  float* Wl = D2 + FC_TM * 60;
  const int tid = threadIdx.x, ti = blockIdx.x, b = blockIdx.y, t0 = ti * FC_TM;
  const int nvalid = min(FC_TM, T - t0);
  const size_t f0 = (size_t)b * T + t0;
  load_tile<20>(Z, z + f0 * 20, nvalid, tid);
  stage_w<40, 20>(Wl, W.w[6], tid);
  __syncthreads();
  for (int e = tid; e < FC_TM * 20; e += FC_NT) {
    const int c = min((20 * t0 + e) / T, 19);                    // (rows behind the utterance: any valid channel)
    ZN[e] = fmaf(Z[e], bnf[40 + c], bnf[60 + c]);
  }
  __syncthreads();
  tile_gemm<20, 40>(ZN, Wl, tid, [&](int m, int n, float v) {
    v = fmaxf(v + W.b[6][n], 0.0f);
    A1[m * 40 + n] = v;
    if (m < nvalid) a1[(f0 + m) * 40 + n] = v;
  });
  __syncthreads();
  stage_w<40, 40>(Wl, W.w[7], tid);
  __syncthreads();
  tile_gemm<40, 40>(A1, Wl, tid, [&](int m, int n, float v) {
    v = fmaxf(v + W.b[7][n], 0.0f);
    U[m * 40 + n] = v;
    if (m < nvalid) u[(f0 + m) * 40 + n] = v;
  });
  __syncthreads();
  // pooling sums of this tile: column c, four strips of 16 rows (fp64), added in order
  if (tid < 160) {
    const int c = tid % 40, s = tid / 40;
    double S = 0.0, Q = 0.0;
    for (int m = 16 * s; m < min(16 * s + 16, nvalid); ++m) { const double v = U[m * 40 + c]; S += v; Q += v * v; }
    red[2 * tid] = S; red[2 * tid + 1] = Q;
  }
  stage_w<40, 20>(Wl, W.w[3], tid);
  __syncthreads();
  if (tid < 80) {
    const int c = tid % 40, comp = tid / 40;
    double v = 0.0;
    for (int s = 0; s < 4; ++s) v += red[2 * (s * 40 + c) + comp];
    poolpart[((size_t)b * gridDim.x + ti) * 80 + comp * 40 + c] = v;
  }
  tile_gemm<20, 40>(Z, Wl, tid, [&](int m, int n, float v) {
    v = fmaxf(v + W.b[3][n], 0.0f);
    A1[m * 40 + n] = v;
    if (m < nvalid) d1[(f0 + m) * 40 + n] = v;
  });
  __syncthreads();
  stage_w<60, 40>(Wl, W.w[4], tid);
  __syncthreads();
  tile_gemm<40, 60>(A1, Wl, tid, [&](int m, int n, float v) {
    v = fmaxf(v + W.b[4][n], 0.0f);
    D2[m * 60 + n] = v;
    if (m < nvalid) d2[(f0 + m) * 60 + n] = v;
  });
  __syncthreads();
  stage_w<80, 60>(Wl, W.w[5], tid);
  __syncthreads();
  tile_gemm<60, 80>(D2, Wl, tid, [&](int m, int n, float v) {
    if (m < nvalid) recon[(f0 + m) * 80 + n] = v + W.b[5][n];
  });
}

// ---------------------------------------------------------------------------------------------------
// inference: recon = decoder(encoder(feats)) in one launch.  The six layers of sa_fc_enc_fwd and of
// sa_fc_mid_fwd's decoder half, through the same tile_gemm instantiations (each output accumulated in the
// same order: the same bits as the train forward's recon); the tile's activations alternate between two
// LDS buffers and only recon leaves the workgroup.  No statistics, no classifier branch.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FC_NT) void fc_recon_fwd_kernel(const float* __restrict__ feats, FcW W,
                                                             float* __restrict__ recon, int T) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* P = reinterpret_cast<float*>(smem);                     // [64][80]: feats, h2 [64][40], d1 [64][40]
  float* Q = P + FC_TM * 80;                                     // [64][80]: h1 [64][60], z [64][20], d2 [64][60]
  float* Wl = Q + FC_TM * 80;
  const int tid = threadIdx.x, ti = blockIdx.x, b = blockIdx.y, t0 = ti * FC_TM;
  const int nvalid = min(FC_TM, T - t0);
  const size_t f0 = (size_t)b * T + t0;
  load_tile<80>(P, feats + f0 * 80, nvalid, tid);
  stage_w<60, 80>(Wl, W.w[0], tid);
  __syncthreads();
  tile_gemm<80, 60>(P, Wl, tid, [&](int m, int n, float v) { Q[m * 60 + n] = fmaxf(v + W.b[0][n], 0.0f); });
  __syncthreads();
  stage_w<40, 60>(Wl, W.w[1], tid);
  __syncthreads();
  tile_gemm<60, 40>(Q, Wl, tid, [&](int m, int n, float v) { P[m * 40 + n] = fmaxf(v + W.b[1][n], 0.0f); });
  __syncthreads();
  stage_w<20, 40>(Wl, W.w[2], tid);
  __syncthreads();
  tile_gemm<40, 20>(P, Wl, tid, [&](int m, int n, float v) { Q[m * 20 + n] = v + W.b[2][n]; });
  __syncthreads();
  stage_w<40, 20>(Wl, W.w[3], tid);
  __syncthreads();
  tile_gemm<20, 40>(Q, Wl, tid, [&](int m, int n, float v) { P[m * 40 + n] = fmaxf(v + W.b[3][n], 0.0f); });
  __syncthreads();
  stage_w<60, 40>(Wl, W.w[4], tid);
  __syncthreads();
  tile_gemm<40, 60>(P, Wl, tid, [&](int m, int n, float v) { Q[m * 60 + n] = fmaxf(v + W.b[4][n], 0.0f); });
  __syncthreads();
  stage_w<80, 60>(Wl, W.w[5], tid);
  __syncthreads();
  tile_gemm<60, 80>(Q, Wl, tid, [&](int m, int n, float v) {
    if (m < nvalid) recon[(f0 + m) * 80 + n] = v + W.b[5][n];
  });
}

// ---------------------------------------------------------------------------------------------------
// the head: pooling finaliser + classify + log_softmax, one workgroup
// ---------------------------------------------------------------------------------------------------
struct FcHead {
  const float *w1, *b1, *g1, *be1; float *rm1, *rv1;            // Linear(80,40), BatchNorm1d(40)
  const float *w2, *b2, *w3, *b3;                               // Linear(40,40), Linear(40,20)
  const float *g2, *be2; float *rm2, *rv2;                      // BatchNorm1d(20)
  const float *w4, *b4;                                         // Linear(20,2)
};

// The head's BatchNorms see B rows (3 in the reference's runs), and rows of one batch are often close to each
// other: |mean| / sigma of a column reaches a few hundred, and every fp32 rounding of (h - mean) or of the folded
// scale / shift is amplified by that ratio.  The statistics and the normalisation of these B x 40 values are
// therefore evaluated in fp64 and rounded once.
// Statistics of column n of H [M][N] (LDS): train -> batch (fp64), eval -> running; mu / r (LDS, fp64)
__device__ __forceinline__ void fc_head_bn_stats(const float* H, int M, int N, int n, const float* run_mean,
                                                 const float* run_var, int train, float eps, double* mu_o, double* r_o,
                                                 double* var_o) {
  double mu, var;
  if (train) {
    double S = 0.0, Q = 0.0;
    for (int m = 0; m < M; ++m) { const double x = H[m * N + n]; S += x; Q += x * x; }
    mu = S / (double)M;
    var = Q / (double)M - mu * mu;
    if (var < 0.0) var = 0.0;
  } else {
    mu = run_mean[n]; var = run_var[n];
  }
  mu_o[n] = mu; r_o[n] = 1.0 / sqrt(var + (double)eps);
  if (var_o) *var_o = var;
}
__device__ __forceinline__ float fc_head_bn_apply(float h, double mu, double r, float gamma, float beta) {
  return (float)(((double)h - mu) * r * (double)gamma + (double)beta);
}
// forward: statistics + running update (momentum, unbiased variance) + f [4][N] (mean, rstd, scale, shift)
__device__ __forceinline__ void fc_head_bn(const float* H, int M, int N, int n, const float* gamma, const float* beta,
                                           float* run_mean, float* run_var, int train, float eps, float momentum,
                                           float* f /* [4][N] global */, double* mu_o, double* r_o) {
  double var;
  fc_head_bn_stats(H, M, N, n, run_mean, run_var, train, eps, mu_o, r_o, &var);
  const double mu = mu_o[n], cnt = (double)M;
  if (train) {
    const double unb = cnt > 1.0 ? var * cnt / (cnt - 1.0) : var;
    run_mean[n] = (1.0f - momentum) * run_mean[n] + momentum * (float)mu;
    run_var[n] = (1.0f - momentum) * run_var[n] + momentum * (float)unb;
  }
  const float r = (float)r_o[n], sc = gamma[n] * r;
  f[n] = (float)mu; f[N + n] = r; f[2 * N + n] = sc; f[3 * N + n] = beta[n] - (float)mu * sc;
}

// out[m][n] = sum_k A[m][k] * W[n][k] + b[n] over M x N outputs (LDS A, pitch K; W global, read through L1)
template <int K, int N, class EP>
__device__ __forceinline__ void head_dense(const float* A, const float* W, const float* bias, int M, int tid, int nthreads,
                                           EP ep) {
  for (int i = tid; i < M * N; i += nthreads) {
    const int m = i / N, n = i % N;
    float acc = 0.0f;
#pragma unroll 4
    for (int k = 0; k < K; ++k) acc = fmaf(A[m * K + k], W[n * K + k], acc);
    ep(m, n, acc + bias[n]);
  }
}

__global__ __launch_bounds__(FC_NT) void fc_head_fwd_kernel(const double* __restrict__ poolpart, int ntile,
                                                            const float* __restrict__ noise, FcHead P, float* pooled,
                                                            float* pst, float* h1, float* f1, float* h2, float* h3,
                                                            float* f2, float* logp, int M, int T, int train, float eps,
                                                            float momentum) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* mu1 = reinterpret_cast<double*>(smem); double* r1 = mu1 + 40; double* mu2 = r1 + 40; double* r2 = mu2 + 20;
  float* X = reinterpret_cast<float*>(r2 + 20);                  // [M][80] pooled
  float* H1 = X + M * 80;                                        // [M][40] Linear 1 (pre-BatchNorm)
  float* A = H1 + M * 40;                                        // [M][40] relu(bn1)
  float* H2 = A + M * 40;                                        // [M][40] relu(Linear 2)
  float* H3 = H2 + M * 40;                                       // [M][20] Linear 3 (pre-BatchNorm)
  float* Y = H3 + M * 20;                                        // [M][20] bn2
  float* lg = Y + M * 20;                                        // [M][2]
  const int tid = threadIdx.x;
  // StatisticsPooling: mean (+ the noise offset eps * ((1 - 9) g + 9)), unbiased std + 1e-5
  for (int i = tid; i < M * 40; i += FC_NT) {
    const int b = i / 40, c = i % 40;
    double S = 0.0, Q = 0.0;
    for (int p = 0; p < ntile; ++p) {
      S += poolpart[((size_t)b * ntile + p) * 80 + c];
      Q += poolpart[((size_t)b * ntile + p) * 80 + 40 + c];
    }
    const double mean = S / (double)T;
    double var = (Q - S * mean) / (double)(T - 1);
    if (var < 0.0) var = 0.0;
    const float mf = (float)mean, sf = (float)sqrt(var);
    pst[b * 80 + c] = mf; pst[b * 80 + 40 + c] = sf;
    float mo = mf;
    if (noise) mo += 1e-5f * ((1.0f - 9.0f) * noise[b * 40 + c] + 9.0f);
    const float so = sf + 1e-5f;
    X[b * 80 + c] = mo; X[b * 80 + 40 + c] = so;
    pooled[b * 80 + c] = mo; pooled[b * 80 + 40 + c] = so;
  }
  __syncthreads();
  head_dense<80, 40>(X, P.w1, P.b1, M, tid, FC_NT, [&](int m, int n, float v) { H1[m * 40 + n] = v; h1[m * 40 + n] = v; });
  __syncthreads();
  if (tid < 40) fc_head_bn(H1, M, 40, tid, P.g1, P.be1, P.rm1, P.rv1, train, eps, momentum, f1, mu1, r1);
  __syncthreads();
  for (int i = tid; i < M * 40; i += FC_NT) {
    const int n = i % 40;
    A[i] = fmaxf(fc_head_bn_apply(H1[i], mu1[n], r1[n], P.g1[n], P.be1[n]), 0.0f);
  }
  __syncthreads();
  head_dense<40, 40>(A, P.w2, P.b2, M, tid, FC_NT, [&](int m, int n, float v) {
    v = fmaxf(v, 0.0f); H2[m * 40 + n] = v; h2[m * 40 + n] = v;
  });
  __syncthreads();
  head_dense<40, 20>(H2, P.w3, P.b3, M, tid, FC_NT, [&](int m, int n, float v) { H3[m * 20 + n] = v; h3[m * 20 + n] = v; });
  __syncthreads();
  if (tid < 20) fc_head_bn(H3, M, 20, tid, P.g2, P.be2, P.rm2, P.rv2, train, eps, momentum, f2, mu2, r2);
  __syncthreads();
  for (int i = tid; i < M * 20; i += FC_NT) {
    const int n = i % 20;
    Y[i] = fc_head_bn_apply(H3[i], mu2[n], r2[n], P.g2[n], P.be2[n]);
  }
  __syncthreads();
  head_dense<20, 2>(Y, P.w4, P.b4, M, tid, FC_NT, [&](int m, int n, float v) { lg[m * 2 + n] = v; });
  __syncthreads();
  if (tid < M * 2) {
    const int m = tid / 2;
    const float x0 = lg[m * 2], x1 = lg[m * 2 + 1], mx = fmaxf(x0, x1);
    const float lse = mx + logf(expf(x0 - mx) + expf(x1 - mx));
    logp[tid] = lg[tid] - lse;
  }
}

// BatchNorm backward of column n over M rows, in fp64 with the forward's statistics recomputed (see above):
// d gamma, d beta, dN (LDS) overwritten with d H.  eval mode (running statistics): d H = gamma * rstd * d N.
__device__ __forceinline__ void fc_head_bn_bwd(float* dN, const float* H, int M, int N, int n, double mu, double r,
                                               const float* gamma, int train, float* dgamma, float* dbeta) {
  double S1 = 0.0, S2 = 0.0;
  for (int m = 0; m < M; ++m) {
    const double g = dN[m * N + n], hh = ((double)H[m * N + n] - mu) * r;
    S1 += g; S2 += g * hh;
  }
  dbeta[n] = (float)S1;
  dgamma[n] = (float)S2;
  const double a1 = train ? S1 / (double)M : 0.0, a2 = train ? S2 / (double)M : 0.0;
  const double c = (double)gamma[n] * r;
  for (int m = 0; m < M; ++m) {
    const double hh = ((double)H[m * N + n] - mu) * r;
    dN[m * N + n] = (float)(c * ((double)dN[m * N + n] - a1 - hh * a2));
  }
}

// d W [N][K] = sum_m D[m][n] * A[m][k]; d b [n] = sum_m D[m][n]  (LDS operands)
template <int N, int K>
__device__ __forceinline__ void head_wgrad(const float* D, const float* A, int M, int tid, int nthreads, float* dW, float* db) {
  for (int i = tid; i < N * K; i += nthreads) {
    const int n = i / K, k = i % K;
    float acc = 0.0f;
    for (int m = 0; m < M; ++m) acc = fmaf(D[m * N + n], A[m * K + k], acc);
    dW[i] = acc;
  }
  for (int n = tid; n < N; n += nthreads) {
    float acc = 0.0f;
    for (int m = 0; m < M; ++m) acc += D[m * N + n];
    db[n] = acc;
  }
}
// d A [m][k] = sum_n D[m][n] * W[n][k]
template <int N, int K, class EP>
__device__ __forceinline__ void head_dgrad(const float* D, const float* W, int M, int tid, int nthreads, EP ep) {
  for (int i = tid; i < M * K; i += nthreads) {
    const int m = i / K, k = i % K;
    float acc = 0.0f;
#pragma unroll 4
    for (int n = 0; n < N; ++n) acc = fmaf(D[m * N + n], W[n * K + k], acc);
    ep(m, k, acc);
  }
}

#define FC_HB_NT 512
// dhead: dw1 3200, db1 40, dg1 40, dbe1 40, dw2 1600, db2 40, dw3 800, db3 20, dg2 20, dbe2 20, dw4 40, db4 2
__global__ __launch_bounds__(FC_HB_NT) void fc_head_bwd_kernel(const float* __restrict__ dlogp, const float* __restrict__ logp,
                                                               const float* __restrict__ pooled, const float* __restrict__ h1,
                                                               const float* __restrict__ h2, const float* __restrict__ h3,
                                                               FcHead P, float* dhead, float* dpooled, int M, int train,
                                                               float eps) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* mu1 = reinterpret_cast<double*>(smem); double* r1 = mu1 + 40; double* mu2 = r1 + 40; double* r2 = mu2 + 20;
  float* X = reinterpret_cast<float*>(r2 + 20);                  // [M][80]
  float* H1 = X + M * 80;                                        // [M][40]
  float* A = H1 + M * 40;                                        // [M][40]
  float* H2 = A + M * 40;                                        // [M][40]
  float* H3 = H2 + M * 40;                                       // [M][20]
  float* Y = H3 + M * 20;                                        // [M][20]
  float* DL = Y + M * 20;                                        // [M][2]
  float* D3 = DL + M * 2;                                        // [M][20] d y -> d h3
  float* D2 = D3 + M * 20;                                       // [M][40] d h2 (masked)
  float* D1 = D2 + M * 40;                                       // [M][40] d a (masked) -> d h1
  const int tid = threadIdx.x;
  float* dw1 = dhead; float* db1 = dw1 + 3200; float* dg1 = db1 + 40; float* dbe1 = dg1 + 40;
  float* dw2 = dbe1 + 40; float* db2 = dw2 + 1600; float* dw3 = db2 + 40; float* db3 = dw3 + 800;
  float* dg2 = db3 + 20; float* dbe2 = dg2 + 20; float* dw4 = dbe2 + 20; float* db4 = dw4 + 40;
  for (int i = tid; i < M * 80; i += FC_HB_NT) X[i] = pooled[i];
  for (int i = tid; i < M * 40; i += FC_HB_NT) { H1[i] = h1[i]; H2[i] = h2[i]; }
  for (int i = tid; i < M * 20; i += FC_HB_NT) H3[i] = h3[i];
  __syncthreads();
  // the forward's statistics and normalised values again, by the forward's own operations (same bits)
  if (tid < 40) fc_head_bn_stats(H1, M, 40, tid, P.rm1, P.rv1, train, eps, mu1, r1, nullptr);
  else if (tid >= 64 && tid < 84) fc_head_bn_stats(H3, M, 20, tid - 64, P.rm2, P.rv2, train, eps, mu2, r2, nullptr);
  __syncthreads();
  for (int i = tid; i < M * 40; i += FC_HB_NT) {
    const int n = i % 40;
    A[i] = fmaxf(fc_head_bn_apply(H1[i], mu1[n], r1[n], P.g1[n], P.be1[n]), 0.0f);
  }
  for (int i = tid; i < M * 20; i += FC_HB_NT) {
    const int n = i % 20;
    Y[i] = fc_head_bn_apply(H3[i], mu2[n], r2[n], P.g2[n], P.be2[n]);
  }
  if (tid < M) {                                                 // d logits = d logp - exp(logp) * sum_c d logp
    const float d0 = dlogp[tid * 2], d1 = dlogp[tid * 2 + 1], s = d0 + d1;
    DL[tid * 2] = d0 - expf(logp[tid * 2]) * s;
    DL[tid * 2 + 1] = d1 - expf(logp[tid * 2 + 1]) * s;
  }
  __syncthreads();
  head_wgrad<2, 20>(DL, Y, M, tid, FC_HB_NT, dw4, db4);
  head_dgrad<2, 20>(DL, P.w4, M, tid, FC_HB_NT, [&](int m, int k, float v) { D3[m * 20 + k] = v; });
  __syncthreads();
  if (tid < 20) fc_head_bn_bwd(D3, H3, M, 20, tid, mu2[tid], r2[tid], P.g2, train, dg2, dbe2);
  __syncthreads();
  head_wgrad<20, 40>(D3, H2, M, tid, FC_HB_NT, dw3, db3);
  head_dgrad<20, 40>(D3, P.w3, M, tid, FC_HB_NT, [&](int m, int k, float v) { D2[m * 40 + k] = H2[m * 40 + k] > 0.0f ? v : 0.0f; });
  __syncthreads();
  head_wgrad<40, 40>(D2, A, M, tid, FC_HB_NT, dw2, db2);
  head_dgrad<40, 40>(D2, P.w2, M, tid, FC_HB_NT, [&](int m, int k, float v) { D1[m * 40 + k] = A[m * 40 + k] > 0.0f ? v : 0.0f; });
  __syncthreads();
  if (tid < 40) fc_head_bn_bwd(D1, H1, M, 40, tid, mu1[tid], r1[tid], P.g1, train, dg1, dbe1);
  __syncthreads();
  head_wgrad<40, 80>(D1, X, M, tid, FC_HB_NT, dw1, db1);
  head_dgrad<40, 80>(D1, P.w1, M, tid, FC_HB_NT, [&](int m, int k, float v) { dpooled[m * 80 + k] = v; });
}

// ---------------------------------------------------------------------------------------------------
// backward 2: decoder (d recon -> d z), pooling + initial (d pooled -> d zn), BatchNorm sums; weight and
// bias gradient partials of decoder.0/2/4 and initial.0/2.  Workgroup g walks tiles g, g + G, ...
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FC_NT) void fc_mid_bwd_kernel(const float* __restrict__ d_recon, const float* __restrict__ dpooled,
                                                           const float* __restrict__ pst, const float* __restrict__ z,
                                                           const float* __restrict__ bnf, const float* __restrict__ a1,
                                                           const float* __restrict__ u, const float* __restrict__ d1,
                                                           const float* __restrict__ d2, FcW W, float* __restrict__ dzn,
                                                           float* __restrict__ dzdec, float* __restrict__ wpart,
                                                           double* __restrict__ bnbpart, int B, int T, int ntile) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* red = reinterpret_cast<double*>(smem);                 // [480]
  double* bnacc = red + 480;                                     // [40]: (sum dy, sum dy * zhat) per channel
  float* P80 = reinterpret_cast<float*>(red + 544);              // [64][80] d recon; later u [64][40] | du [64][40]
  float* Q60a = P80 + FC_TM * 80;                                // [64][60] d2; later a1 [64][40]
  float* Q60b = Q60a + FC_TM * 60;                               // [64][60] d d2; later d a1 [64][40]
  float* Q40a = Q60b + FC_TM * 60;                               // [64][40] d1
  float* Q40b = Q40a + FC_TM * 40;                               // [64][40] d d1
  float* Z = Q40b + FC_TM * 40;                                  // [64][20]
  float* ZN = Z + FC_TM * 20;                                    // [64][20]
  float* G20 = ZN + FC_TM * 20;                                  // [64][20] d z (decoder), then d zn
  float* Wl = G20 + FC_TM * 20;
  float* pk = Wl + WL_FLOATS;                                    // [2][40] pooling backward coefficients
  const int tid = threadIdx.x, g = blockIdx.x, G = gridDim.x;
  WgAcc<80, 60> w6; WgAcc<60, 40> w5; WgAcc<40, 20> w4; WgAcc<40, 40> wi2; WgAcc<40, 20> wi0;
  w6.zero(); w5.zero(); w4.zero(); wi2.zero(); wi0.zero();
  float b6 = 0.0f, b5 = 0.0f, b4 = 0.0f, bi2 = 0.0f, bi0 = 0.0f;
  if (tid < 40) bnacc[tid] = 0.0;
  for (int q = g; q < B * ntile; q += G) {
    const int b = q / ntile, t0 = (q % ntile) * FC_TM;
    const int nvalid = min(FC_TM, T - t0);
    const size_t f0 = (size_t)b * T + t0;
    __syncthreads();
    load_tile<80>(P80, d_recon + f0 * 80, nvalid, tid);
    load_tile<60>(Q60a, d2 + f0 * 60, nvalid, tid);
    load_tile<40>(Q40a, d1 + f0 * 40, nvalid, tid);
    load_tile<20>(Z, z + f0 * 20, nvalid, tid);
    stage_wt<80, 60>(Wl, W.w[5], tid);
    __syncthreads();
    // ---- decoder ----
    w6.add(P80, Q60a, tid);
    bias_add<80>(b6, P80, tid);
    tile_gemm<80, 60>(P80, Wl, tid, [&](int m, int n, float v) { Q60b[m * 60 + n] = Q60a[m * 60 + n] > 0.0f ? v : 0.0f; });
    __syncthreads();
    stage_wt<60, 40>(Wl, W.w[4], tid);
    w5.add(Q60b, Q40a, tid);
    bias_add<60>(b5, Q60b, tid);
    __syncthreads();
    tile_gemm<60, 40>(Q60b, Wl, tid, [&](int m, int n, float v) { Q40b[m * 40 + n] = Q40a[m * 40 + n] > 0.0f ? v : 0.0f; });
    __syncthreads();
    stage_wt<40, 20>(Wl, W.w[3], tid);
    w4.add(Q40b, Z, tid);
    bias_add<40>(b4, Q40b, tid);
    __syncthreads();
    tile_gemm<40, 20>(Q40b, Wl, tid, [&](int m, int n, float v) {
      if (m < nvalid) dzdec[(f0 + m) * 20 + n] = v;
    });
    __syncthreads();
    // ---- classifier: StatisticsPooling and initial ----
    float* U = P80; float* DU = P80 + FC_TM * 40; float* A1 = Q60a; float* DA1 = Q60b;
    load_tile<40>(U, u + f0 * 40, nvalid, tid);
    load_tile<40>(A1, a1 + f0 * 40, nvalid, tid);
    stage_wt<40, 40>(Wl, W.w[7], tid);
    if (tid < 40) {
      // d u = d mean / T + d std * (u - mean) / ((T - 1) std); torch's std backward gives 0 where std == 0
      const float sd = pst[b * 80 + 40 + tid];
      pk[tid] = dpooled[b * 80 + tid] / (float)T;
      pk[40 + tid] = sd > 0.0f ? dpooled[b * 80 + 40 + tid] / ((float)(T - 1) * sd) : 0.0f;
    }
    for (int e = tid; e < FC_TM * 20; e += FC_NT) {
      const int c = min((20 * t0 + e) / T, 19);
      ZN[e] = fmaf(Z[e], bnf[40 + c], bnf[60 + c]);
    }
    __syncthreads();
    for (int i = tid; i < FC_TM * 40; i += FC_NT) {
      const int m = i / 40, c = i % 40;
      const float uv = U[i];
      DU[i] = (m < nvalid && uv > 0.0f) ? fmaf(pk[40 + c], uv - pst[b * 80 + c], pk[c]) : 0.0f;
    }
    __syncthreads();
    wi2.add(DU, A1, tid);
    bias_add<40>(bi2, DU, tid);
    tile_gemm<40, 40>(DU, Wl, tid, [&](int m, int n, float v) { DA1[m * 40 + n] = A1[m * 40 + n] > 0.0f ? v : 0.0f; });
    __syncthreads();
    stage_wt<40, 20>(Wl, W.w[6], tid);
    wi0.add(DA1, ZN, tid);
    bias_add<40>(bi0, DA1, tid);
    __syncthreads();
    tile_gemm<40, 20>(DA1, Wl, tid, [&](int m, int n, float v) {
      G20[m * 20 + n] = v;
      if (m < nvalid) dzn[(f0 + m) * 20 + n] = v;
    });
    __syncthreads();
    tile_chan_sums(T, t0, nvalid, tid, red,
                   [&](int e, int c, double& a, double& s) {
                     const float dy = G20[e], zh = (Z[e] - bnf[c]) * bnf[20 + c];
                     a += dy; s += (double)dy * zh;
                   },
                   [&](int c, int comp, double v) { bnacc[2 * c + comp] += v; });
  }
  __syncthreads();
  float* wp = wpart + (size_t)g * FC_NPARAM;
  w4.store(wp + WOFF<3>, tid); w5.store(wp + WOFF<4>, tid); w6.store(wp + WOFF<5>, tid);
  wi0.store(wp + WOFF<6>, tid); wi2.store(wp + WOFF<7>, tid);
  if (tid < 40) { wp[BOFF<3> + tid] = b4; wp[BOFF<6> + tid] = bi0; wp[BOFF<7> + tid] = bi2; }
  if (tid < 60) wp[BOFF<4> + tid] = b5;
  if (tid < 80) wp[BOFF<5> + tid] = b6;
  if (tid < 40) bnbpart[(size_t)g * 40 + tid] = bnacc[tid];
}

// ---------------------------------------------------------------------------------------------------
// backward 3: BatchNorm1d(20) backward coefficients with GradReverse folded in:
//   d z (classifier branch) = -(gamma rstd (dy - S1/n - zhat S2/n)) = c1 dy + c2 z + c3;  d gamma = S2, d beta = S1
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FC_NT) void fc_bn_bwd_fin_kernel(const double* __restrict__ bnbpart, int npart,
                                                              const float* gamma, const float* bnf, float* coef,
                                                              float* dgamma, float* dbeta, double count, int train) {
  __shared__ double red[240];
  const int tid = threadIdx.x;
  if (tid < 240) {
    const int v = tid % 40, s = tid / 40;
    double a = 0.0;
    for (int p = s; p < npart; p += 6) a += bnbpart[(size_t)p * 40 + v];
    red[tid] = a;
  }
  __syncthreads();
  if (tid < 20) {
    double S1 = 0.0, S2 = 0.0;
    for (int s = 0; s < 6; ++s) { S1 += red[s * 40 + 2 * tid]; S2 += red[s * 40 + 2 * tid + 1]; }
    dbeta[tid] = (float)S1; dgamma[tid] = (float)S2;
    const double mu = bnf[tid], r = bnf[20 + tid], gr = (double)gamma[tid] * r;
    const double c2 = train ? gr * r * S2 / count : 0.0;
    const double c3 = train ? gr * S1 / count - c2 * mu : 0.0;
    coef[tid] = (float)(-gr); coef[20 + tid] = (float)c2; coef[40 + tid] = (float)c3;
  }
}

// ---------------------------------------------------------------------------------------------------
// backward 4: encoder.  d z = d z (decoder) + c1 d zn + c2 z + c3 -> weight and bias gradient partials of
// encoder.0/2/4 (no gradient to feats)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FC_NT) void fc_enc_bwd_kernel(const float* __restrict__ feats, const float* __restrict__ h1,
                                                           const float* __restrict__ h2, const float* __restrict__ z,
                                                           const float* __restrict__ dzn, const float* __restrict__ dzdec,
                                                           const float* __restrict__ coef, FcW W, float* __restrict__ wpart,
                                                           int B, int T, int ntile) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* X = reinterpret_cast<float*>(smem);                     // [64][80]
  float* H1 = X + FC_TM * 80;                                    // [64][60]
  float* DH1 = H1 + FC_TM * 60;                                  // [64][60]
  float* H2 = DH1 + FC_TM * 60;                                  // [64][40]
  float* DH2 = H2 + FC_TM * 40;                                  // [64][40]
  float* DZ = DH2 + FC_TM * 40;                                  // [64][20]
  float* Wl = DZ + FC_TM * 20;
  const int tid = threadIdx.x, g = blockIdx.x, G = gridDim.x;
  WgAcc<60, 80> w1; WgAcc<40, 60> w2; WgAcc<20, 40> w3;
  w1.zero(); w2.zero(); w3.zero();
  float b1 = 0.0f, b2 = 0.0f, b3 = 0.0f;
  for (int q = g; q < B * ntile; q += G) {
    const int b = q / ntile, t0 = (q % ntile) * FC_TM;
    const int nvalid = min(FC_TM, T - t0);
    const size_t f0 = (size_t)b * T + t0;
    __syncthreads();
    load_tile<80>(X, feats + f0 * 80, nvalid, tid);
    load_tile<60>(H1, h1 + f0 * 60, nvalid, tid);
    load_tile<40>(H2, h2 + f0 * 40, nvalid, tid);
    for (int e = tid; e < FC_TM * 20; e += FC_NT) {
      float v = 0.0f;
      if (e < 20 * nvalid) {
        const int c = (20 * t0 + e) / T;
        const size_t i = f0 * 20 + e;
        v = dzdec[i] + fmaf(coef[c], dzn[i], fmaf(coef[20 + c], z[i], coef[40 + c]));
      }
      DZ[e] = v;
    }
    stage_wt<20, 40>(Wl, W.w[2], tid);
    __syncthreads();
    w3.add(DZ, H2, tid);
    bias_add<20>(b3, DZ, tid);
    tile_gemm<20, 40>(DZ, Wl, tid, [&](int m, int n, float v) { DH2[m * 40 + n] = H2[m * 40 + n] > 0.0f ? v : 0.0f; });
    __syncthreads();
    stage_wt<40, 60>(Wl, W.w[1], tid);
    w2.add(DH2, H1, tid);
    bias_add<40>(b2, DH2, tid);
    __syncthreads();
    tile_gemm<40, 60>(DH2, Wl, tid, [&](int m, int n, float v) { DH1[m * 60 + n] = H1[m * 60 + n] > 0.0f ? v : 0.0f; });
    __syncthreads();
    w1.add(DH1, X, tid);
    bias_add<60>(b1, DH1, tid);
  }
  float* wp = wpart + (size_t)g * FC_NPARAM;
  w1.store(wp + WOFF<0>, tid); w2.store(wp + WOFF<1>, tid); w3.store(wp + WOFF<2>, tid);
  if (tid < 60) wp[BOFF<0> + tid] = b1;
  if (tid < 40) wp[BOFF<1> + tid] = b2;
  if (tid < 20) wp[BOFF<2> + tid] = b3;
}

// backward 5: the G workgroup partials added in order (fp64) -> the 16 gradients in nn.Linear layout
__global__ __launch_bounds__(FC_NT) void fc_wreduce_kernel(const float* __restrict__ wpart, int G, float* __restrict__ grads) {
  const int i = blockIdx.x * FC_NT + threadIdx.x;
  if (i >= FC_NPARAM) return;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += wpart[(size_t)g * FC_NPARAM + i];
  grads[i] = (float)s;
}

constexpr size_t LDS_ENC_FWD = fc_lds(200), LDS_MID_FWD = fc_lds(180);
constexpr size_t LDS_MID_BWD = fc_lds(340) + 80 * sizeof(float), LDS_ENC_BWD = fc_lds(300);
// two activation buffers of 64 x 80 floats + one staged matrix, without the fp64 reduction scratch of fc_lds()
constexpr size_t LDS_RECON = ((size_t)FC_TM * 160 + WL_FLOATS) * sizeof(float);
static_assert(LDS_RECON + 544 * sizeof(double) == fc_lds(160), "sa_fc_recon_fwd: LDS layout");

template <class KERN>
int fc_allow_lds(KERN kern, bool& done) {
  if (!done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024);
    if (e != hipSuccess) return -(int)e;
    done = true;
  }
  return 0;
}

inline int fc_last() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}

inline FcW fc_w(const void* const* wb) {
  FcW W;
  for (int i = 0; i < 8; ++i) { W.w[i] = static_cast<const float*>(wb[i]); W.b[i] = static_cast<const float*>(wb[8 + i]); }
  return W;
}
inline bool fc_all(const void* const* p, int n) {
  if (!p) return false;
  for (int i = 0; i < n; ++i)
    if (!p[i]) return false;
  return true;
}
inline FcHead fc_head(const void* const* hw) {
  auto c = [&](int i) { return static_cast<const float*>(hw[i]); };
  auto m = [&](int i) { return static_cast<float*>(const_cast<void*>(hw[i])); };
  return FcHead{c(0), c(1), c(2), c(3), m(4), m(5), c(6), c(7), c(8), c(9), c(10), c(11), m(12), m(13), c(14), c(15)};
}
inline bool fc_shape_ok(int B, int T) { return B >= 1 && T >= 2 && (long long)B * T * 80 < (1ll << 31); }
// the reconstruction alone has no pooling (T - 1) and no head: one frame is enough, and B is the grid's y extent
inline bool fc_recon_shape_ok(int B, int T) { return B >= 1 && B <= 65535 && T >= 1 && (long long)B * T * 80 < (1ll << 31); }

}  // namespace

extern "C" int sa_fc_tiles(int T) { return T < 1 ? -22 : sa_div_up(T, FC_TM); }
extern "C" int sa_fc_groups(int B, int T) {
  if (!fc_shape_ok(B, T)) return -22;
  const long long n = (long long)B * sa_div_up(T, FC_TM);
  return (int)(n < FC_MAXG ? n : FC_MAXG);
}
extern "C" int sa_fc_nparam(void) { return FC_NPARAM; }
extern "C" int sa_fc_nhead(void) { return FC_NHEAD; }
extern "C" int sa_fc_max_rows(void) { return FC_MAXB; }

extern "C" int sa_fc_enc_fwd(const float* feats, const void* const* wb, float* h1, float* h2, float* z, double* bnpart,
                             int B, int T, void* stream) {
  if (!feats || !fc_all(wb, 16) || !h1 || !h2 || !z || !bnpart || !fc_shape_ok(B, T)) return -22;
  static bool ok = false;
  if (int rc = fc_allow_lds(fc_enc_fwd_kernel, ok)) return rc;
  hipLaunchKernelGGL(fc_enc_fwd_kernel, dim3(sa_div_up(T, FC_TM), B), dim3(FC_NT), LDS_ENC_FWD,
                     reinterpret_cast<hipStream_t>(stream), feats, fc_w(wb), h1, h2, z, bnpart, T);
  return fc_last();
}

extern "C" int sa_fc_bn_fin(const double* bnpart, int npart, const float* gamma, const float* beta, float* run_mean,
                            float* run_var, float* bnf, int B, int T, int train, float eps, float momentum, void* stream) {
  if (!gamma || !beta || !run_mean || !run_var || !bnf || !fc_shape_ok(B, T) || (train && (!bnpart || npart < 1))) return -22;
  hipLaunchKernelGGL(fc_bn_fin_kernel, dim3(1), dim3(FC_NT), 0, reinterpret_cast<hipStream_t>(stream), bnpart, npart, gamma,
                     beta, run_mean, run_var, bnf, (double)B * T, train, eps, momentum);
  return fc_last();
}

extern "C" int sa_fc_mid_fwd(const float* z, const float* bnf, const void* const* wb, float* a1, float* u, float* d1,
                             float* d2, float* recon, double* poolpart, int B, int T, void* stream) {
  if (!z || !bnf || !fc_all(wb, 16) || !a1 || !u || !d1 || !d2 || !recon || !poolpart || !fc_shape_ok(B, T)) return -22;
  static bool ok = false;
  if (int rc = fc_allow_lds(fc_mid_fwd_kernel, ok)) return rc;
  hipLaunchKernelGGL(fc_mid_fwd_kernel, dim3(sa_div_up(T, FC_TM), B), dim3(FC_NT), LDS_MID_FWD,
                     reinterpret_cast<hipStream_t>(stream), z, bnf, fc_w(wb), a1, u, d1, d2, recon, poolpart, T);
  return fc_last();
}

extern "C" int sa_fc_recon_fwd(const float* feats, const void* const* wb, float* recon, int B, int T, void* stream) {
  if (!feats || !fc_all(wb, 16) || !recon || !fc_recon_shape_ok(B, T)) return -22;
  static bool ok = false;
  if (int rc = fc_allow_lds(fc_recon_fwd_kernel, ok)) return rc;
  hipLaunchKernelGGL(fc_recon_fwd_kernel, dim3(sa_div_up(T, FC_TM), B), dim3(FC_NT), LDS_RECON,
                     reinterpret_cast<hipStream_t>(stream), feats, fc_w(wb), recon, T);
  return fc_last();
}

extern "C" int sa_fc_head_fwd(const double* poolpart, const float* noise, const void* const* hw, float* pooled, float* pst,
                              float* h1, float* f1, float* h2, float* h3, float* f2, float* logp, int B, int T, int train,
                              float eps, float momentum, void* stream) {
  if (!poolpart || !fc_all(hw, 16) || !pooled || !pst || !h1 || !f1 || !h2 || !h3 || !f2 || !logp || !fc_shape_ok(B, T) ||
      B > FC_MAXB)
    return -22;
  static bool ok = false;
  if (int rc = fc_allow_lds(fc_head_fwd_kernel, ok)) return rc;
  const size_t lds = (size_t)B * 242 * sizeof(float) + 120 * sizeof(double);
  hipLaunchKernelGGL(fc_head_fwd_kernel, dim3(1), dim3(FC_NT), lds, reinterpret_cast<hipStream_t>(stream), poolpart,
                     sa_div_up(T, FC_TM), noise, fc_head(hw), pooled, pst, h1, f1, h2, h3, f2, logp, B, T, train, eps, momentum);
  return fc_last();
}

extern "C" int sa_fc_head_bwd(const float* dlogp, const float* logp, const float* pooled, const float* h1,
                              const float* h2, const float* h3, const void* const* hw, float* dhead,
                              float* dpooled, int B, int train, float eps, void* stream) {
  if (!dlogp || !logp || !pooled || !h1 || !h2 || !h3 || !fc_all(hw, 16) || !dhead || !dpooled || B < 1 ||
      B > FC_MAXB)
    return -22;
  static bool ok = false;
  if (int rc = fc_allow_lds(fc_head_bwd_kernel, ok)) return rc;
  const size_t lds = (size_t)B * 342 * sizeof(float) + 120 * sizeof(double);
  hipLaunchKernelGGL(fc_head_bwd_kernel, dim3(1), dim3(FC_HB_NT), lds, reinterpret_cast<hipStream_t>(stream), dlogp, logp,
                     pooled, h1, h2, h3, fc_head(hw), dhead, dpooled, B, train, eps);
  return fc_last();
}

extern "C" int sa_fc_mid_bwd(const float* d_recon, const float* dpooled, const float* pst, const float* z, const float* bnf,
                             const float* a1, const float* u, const float* d1, const float* d2, const void* const* wb,
                             float* dzn, float* dzdec, float* wpart, double* bnbpart, int B, int T, void* stream) {
  if (!d_recon || !dpooled || !pst || !z || !bnf || !a1 || !u || !d1 || !d2 || !fc_all(wb, 16) || !dzn || !dzdec || !wpart ||
      !bnbpart || !fc_shape_ok(B, T))
    return -22;
  static bool ok = false;
  if (int rc = fc_allow_lds(fc_mid_bwd_kernel, ok)) return rc;
  hipLaunchKernelGGL(fc_mid_bwd_kernel, dim3(sa_fc_groups(B, T)), dim3(FC_NT), LDS_MID_BWD,
                     reinterpret_cast<hipStream_t>(stream), d_recon, dpooled, pst, z, bnf, a1, u, d1, d2, fc_w(wb), dzn, dzdec,
                     wpart, bnbpart, B, T, sa_div_up(T, FC_TM));
  return fc_last();
}

extern "C" int sa_fc_bn_bwd_fin(const double* bnbpart, int npart, const float* gamma, const float* bnf, float* coef,
                                float* dgamma, float* dbeta, int B, int T, int train, void* stream) {
  if (!bnbpart || npart < 1 || !gamma || !bnf || !coef || !dgamma || !dbeta || !fc_shape_ok(B, T)) return -22;
  hipLaunchKernelGGL(fc_bn_bwd_fin_kernel, dim3(1), dim3(FC_NT), 0, reinterpret_cast<hipStream_t>(stream), bnbpart, npart,
                     gamma, bnf, coef, dgamma, dbeta, (double)B * T, train);
  return fc_last();
}

extern "C" int sa_fc_enc_bwd(const float* feats, const float* h1, const float* h2, const float* z, const float* dzn,
                             const float* dzdec, const float* coef, const void* const* wb, float* wpart, int B, int T,
                             void* stream) {
  if (!feats || !h1 || !h2 || !z || !dzn || !dzdec || !coef || !fc_all(wb, 16) || !wpart || !fc_shape_ok(B, T)) return -22;
  static bool ok = false;
  if (int rc = fc_allow_lds(fc_enc_bwd_kernel, ok)) return rc;
  hipLaunchKernelGGL(fc_enc_bwd_kernel, dim3(sa_fc_groups(B, T)), dim3(FC_NT), LDS_ENC_BWD,
                     reinterpret_cast<hipStream_t>(stream), feats, h1, h2, z, dzn, dzdec, coef, fc_w(wb), wpart, B, T,
                     sa_div_up(T, FC_TM));
  return fc_last();
}

extern "C" int sa_fc_wreduce(const float* wpart, int G, float* grads, void* stream) {
  if (!wpart || G < 1 || !grads) return -22;
  hipLaunchKernelGGL(fc_wreduce_kernel, dim3(sa_div_up(FC_NPARAM, FC_NT)), dim3(FC_NT), 0, reinterpret_cast<hipStream_t>(stream),
                     wpart, G, grads);
  return fc_last();
}
