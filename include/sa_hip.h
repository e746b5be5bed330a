/* sa_hip.h -- C ABI of libsa_hip.so, the MI355X (gfx950) compute library behind the
 * speech-anonymization ConvAE + gender-adversarial train step.
 *
 * The reference (viswavi/speech-anonymization) has no native / FFI boundary: the hot path is
 * PyTorch ops reached from three Python seams.  This header is the boundary a
 * maintainer binds instead (ctypes stub: INTEGRATION.md); each entry point cites the
 * reference code whose arithmetic it replaces.  Conventions:
 *   - plain C: pointers + sizes, no torch / HIP types; `stream` is a hipStream_t passed as void*
 *     (torch.cuda.current_stream().cuda_stream); every call only ENQUEUES work on it;
 *   - every buffer (inputs, outputs, saved tensors, workspaces) is caller-allocated device
 *     memory; the library allocates nothing and keeps no state besides kernel attributes --
 *     except, per process, ONE RCCL communicator + one side stream + two events between
 *     sa_comm_init and sa_comm_destroy (data-parallel exchange, at the end of this header);
 *   - return 0 on success, -EINVAL (-22) for bad arguments, -ENOSYS (-38) for a shape that is
 *     not instantiated, or -(hipError_t) from the launch; nothing throws across the ABI;
 *   - dtype: SA_F32 (0) or SA_BF16 (1) = storage type of activations and packed weights;
 *     accumulation and all statistics are fp32 (fp64 in the tiny finalisers);
 *   - activations are CHANNELS-LAST [B][L][C]; the reference's [B][C][L] tensors are never
 *     materialised (C = 1 at both ends of the auto-encoder, so the module boundary
 *     feats[B][T][80] -> recon[B][T][80] needs no conversion).
 */
#ifndef SA_HIP_H
#define SA_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define SA_F32 0
#define SA_BF16 1
#define SA_BF16X3 2   /* fp32 storage, split-bf16 operands, 3 bf16 MFMAs per k-step */
#define SA_BF16X1F 3  /* fp32 storage, operands rounded to bf16 once, 1 bf16 MFMA (sa_wgrad only) */
#define SA_FP8 4      /* FORWARD-OPERAND EXPERIMENT, not a training mode and not BASELINE config 5 (which is
                       * listed as not built: DESIGN.md 3): bf16 storage; MFMA operands OCP e4m3 -- the
                       * activation rows are quantised unscaled while they are staged, the weight image is
                       * e4m3 scaled by a per-tensor power of two (SaConvArgs.wscale, undone in the
                       * epilogue); fp32 accumulation and statistics.  Forward-type launches of
                       * sa_conv_gemm only; gradients stay on SA_BF16.  Measured: same speed as SA_BF16
                       * (the non-scaled K = 16 fp8 MFMA runs at the bf16 rate), reconstruction 2.4e-2
                       * off the fp32 oracle, the adversarial (classifier-branch) gradient direction lost
                       * (cosine 0.13).  Kept because the kernel is exact against emulated e4m3 operands
                       * (tests) and pins the e4m3 fragment layout for a block-scaled follow-up. */
#define SA_F64 5      /* sa_comm_allreduce only: the SyncBatchNorm element counts */
#define SA_MAX_TAPS 5
#define SA_COMM_ID_BYTES 128

/* ---- implicit-GEMM convolution (sa_conv_gemm.hip) -------------------------------------
 * Row-gather GEMM covering nn.Conv1d, nn.ConvTranspose1d(stride 2) and both data gradients
 * (models/ConvAutoEncoder.py:141-172 encoder/decoder, :33-43 TDNN; backward via
 * speechbrain_convae_train.py:241).  For base row m and phase ph < U the output row is
 * o = m*U + ph and
 *   y[b,o,co] = bias[co] + sum_{t<ntaps[ph]} sum_ci P(x)[b, m*SA + off[ph][t], ci] * W[widx[ph][t]][ci][co]
 * rows outside [0,Lin) are zero.  P = prologue: v*s1[b][ci]+t1[b][ci] -> x*sigmoid(x) if swish
 * -> v*s2[ci]+t2[ci] (any pointer may be NULL).  Epilogue: +bias, ReLU if relu, store, and if
 * stats != NULL per-tile partial (sum, sumsq) of the stored values -> stats[B][ntiles][COUT][2]
 * with ntiles = sa_conv_gemm_ntiles(cin, cout, u, Lout). */
typedef struct SaTaps {
  int ntaps[2];
  int off[2][SA_MAX_TAPS];
  int widx[2][SA_MAX_TAPS];
} SaTaps;

typedef struct SaConvArgs {
  const void* x;
  const void* wp;            /* sa_pack_weights image */
  const float* bias;
  void* y;
  const float* s1; const float* t1;
  const float* s2; const float* t2;
  int swish;
  int relu;
  float* stats;
  int B, Lin, Lout, ntiles;  /* ntiles, rowmin, nrows, wlo_off are filled in by the library */
  int rowmin, nrows, wlo_off;
  SaTaps taps;
  /* fused backward epilogue (dgrad launches): ep_mode 0 = off; 1 = g' = (acc + ep_g2) * swish'(z),
   * z = ep_x*ep_s1[b][c] + ep_t1[b][c]; 2 = g' = acc + ep_g2.  g' is what is stored in y, and stats
   * becomes (sum g', sum g'*xhat), xhat = (xv - ep_mean)*ep_rstd with xv = ep_x, or swish(z) when
   * ep_xp_is_act; ep_mean / ep_rstd are indexed [b*ep_bstride + c] (ep_bstride = COUT or 0). */
  int ep_mode, ep_xp_is_act, ep_bstride;
  const void* ep_x; const void* ep_g2;
  const float* ep_s1; const float* ep_t1; const float* ep_mean; const float* ep_rstd;
  /* optional second output: the transformed input rows P(x) = s2*act(s1*x+t1)+t2, rounded to bf16,
   * [B][Lin][CIN] -- what sa_wgrad multiplies with when SaWgradArgs.x_pre is set */
  void* a_out;
  /* normalisation-backward prologue (optional, SA_BF16X3 and SA_BF16 launches): x holds d z of the layer
   * above and nb_x its stored forward tensor y (same shape); the staged rows become
   * d y = nb_c1*dz + nb_c2*y + nb_c3 [zeroed where y <= 0 if nb_relu_mask], coefficients indexed
   * [b*nb_bstride + c] (nb_bstride = CIN or 0); s1..swish are ignored.  This is sa_ew_apply fused
   * into its consumer; with a_out the bf16 d y also feeds sa_wgrad (dy_pre).  nb_colsum
   * [B][ntiles][CIN]: per-tile column sums of d y (bias gradient of the layer below). */
  const void* nb_x; const float* nb_c1; const float* nb_c2; const float* nb_c3;
  int nb_bstride, nb_relu_mask; float* nb_colsum;
  /* optional (ep_mode with ep_g2): ep_g2 is d(BN output) of a BatchNorm over the activation
   * swish(z); the epilogue uses k1[c]*ep_g2 + k2[c]*swish(z) + k3[c] in its place */
  const float* ep_g2k1; const float* ep_g2k2; const float* ep_g2k3;
  /* optional, launches with s1/t1 + swish and no s2: per-tile (sum, sum of squares) of the
   * transformed input rows P(x), [B][ntiles][CIN][2] */
  float* pro_stats;
  /* SA_FP8: device scalar the e4m3 weight image was multiplied with (accumulators are divided by it) */
  const float* wscale;
  /* output rows per workgroup of THIS launch on the one-tile kernel: 0 = the per-shape policy, 64 or
   * 128 (size `stats` with sa_conv_gemm_ntiles_tm) */
  int tile_rows; int pad2_;
} SaConvArgs;

int sa_conv_gemm(int dtype, int cin, int cout, int sa, int u, const SaConvArgs* a, void* stream);
/* sizeof(SaConvArgs | SaWgradArgs | SaEwArgs | SaPackDesc | SaTaps | SaBiasMulti | SaWredMulti | SaFlats) for which = 0..7: lets a binding
 * verify its mirror of these records (the library reads every field) */
int sa_abi_sizeof(int which);
/* ntiles: slabs per utterance of `stats`, nb_colsum and pro_stats -- one per tile, whichever kernel serves
 * the launch; the reducers sum slabs in index order */
int sa_conv_gemm_ntiles(int cin, int cout, int u, int Lout);
int sa_conv_gemm_ntiles_tm(int tile_rows, int u, int Lout);       /* tiles per utterance at an explicit tile height */
int sa_conv_gemm_set_tile_rows(int rows);   /* tuning knob: 0 (default policy), 64 or 128 */
/* Kernel choice of sa_conv_gemm, process-wide.  2 (default): the weight-stationary kernel
 * (sa_conv_ws.hip) serves the bf16x3 128->128, 64->64 stride-1, 64->128 stride-2 and 128->64 / 64->32 transposed launches with >= 1536 tiles that it
 * covers (5 taps at unit spacing, 128 channels also 3 taps over 4 / 6 rows; no fused backward
 * epilogue, no normalisation-backward prologue), sa_conv_wsd.hip the fused 128->128 data gradients under the
 * same condition, the one-tile-per-workgroup kernel everything else -- same geometry and, given the same
 * inputs, the same output bits.  0: one-tile kernel only.  Any other value: -22. */
int sa_conv_gemm_set_impl(int impl);
/* which kernel serves this launch under the current choice: 0 one-tile, 2 weight-stationary, 3 weight-stationary
 * fused data gradient (profiling tools name the kernel they time with it; 1 named a kernel that was removed) */
int sa_conv_gemm_route(int dtype, int cin, int cout, int sa, int u, const SaConvArgs* a);

/* fp32 master weights -> fragment-major MFMA operand image (K = GEMM reduction channels,
 * N = produced channels; element W(t,k,n) = src[k*sk + n*sn + t*st]).
 * nn.Conv1d.weight [Cout][Cin][Kw]: forward sk=Kw, sn=Cin*Kw, st=1; dgrad sk=Cin*Kw, sn=Kw.
 * nn.ConvTranspose1d.weight [Cin][Cout][Kw]: forward sk=Cout*Kw, sn=Kw; dgrad sk=Kw, sn=Cout*Kw. */
int sa_pack_weights(int dtype, const float* src, void* dst, int ntaps, int K, int N, int sk, int sn,
                    int st, void* stream);

/* n images in one launch: descs is an array of n records in DEVICE memory (the record of image i
 * holds the arguments sa_pack_weights would take for it). */
typedef struct SaPackDesc {
  const float* src; void* dst;
  int dtype, ntaps, K, N, sk, sn, st, pad_;
  float* scale;          /* SA_FP8 images: device scalar, written by sa_pack_scales_multi, read by the packer */
} SaPackDesc;
int sa_pack_weights_multi(const SaPackDesc* descs, int n, int blocks_per_image, void* stream);
/* per-tensor power-of-two scale of every SA_FP8 image of the table: 2^floor(log2(448 / max|w|))
 * (one workgroup per image; run it before sa_pack_weights_multi) */
int sa_pack_scales_multi(const SaPackDesc* descs, int n, void* stream);

/* ---- weight gradients (sa_wgrad.hip) --------------------------------------------------
 * dW[t][ci][co] = sum_b sum_{m<Mrows} P(x)[b, m*SA+off[t], ci] * dy[b, m*U+ph[t], co];
 * grid nchunk*B: each workgroup covers `chunk` (multiple of 64) base rows, every tap and the
 * whole CIN x COUT block; slabs[b][chunk][kw][t][CIN][COUT] with
 * kw < sa_wgrad_kw(cin, cout); sa_wgrad_reduce sums the B*nchunk*kw slabs in a fixed order into
 * dst[ci*sk + co*sn + t*st]. */
typedef struct SaWgradArgs {
  const void* x;
  const void* dy;
  float* slabs;
  const float* s1; const float* t1; const float* s2; const float* t2; int swish;
  int B, Lin, Ldy, Mrows, chunk, nchunk;
  int ntaps; int off[SA_MAX_TAPS]; int ph[SA_MAX_TAPS];
  int x_pre;   /* x is SaConvArgs.a_out of the forward launch (bf16, already transformed; s1..swish
                * ignored).  SA_BF16X1F and SA_BF16. */
  int dy_pre;  /* dy is SaConvArgs.a_out of the data-gradient launch that consumed it (bf16 d y);
                * requires x_pre. */
} SaWgradArgs;

int sa_wgrad(int dtype, int cin, int cout, int sa, int u, const SaWgradArgs* a, void* stream);
int sa_wgrad_kw(int cin, int cout);
int sa_wgrad_reduce(const float* slabs, float* dst, int nslab, int ntaps, int cin, int cout, int sk,
                    int sn, int st, int accumulate, void* stream);
/* the reducers of up to SA_WRED_MAX weight gradients in one launch (the end of a backward stage): each record is
 * the argument list of sa_wgrad_reduce (vec is filled in by the library); same order, same bits */
#define SA_WRED_MAX 8
typedef struct SaWredDesc {
  const float* slabs; float* dst;
  int nslab, ntaps, cin, cout, sk, sn, st, accumulate, vec, pad_;
} SaWredDesc;
typedef struct SaWredMulti { int n, pad_; SaWredDesc d[SA_WRED_MAX]; } SaWredMulti;
int sa_wgrad_reduce_multi(const SaWredMulti* m, void* stream);

/* ---- single-channel ends (sa_small.hip): encoder.0 Conv1d(1,32,15,p7) / decoder.8
 * Conv1d(32,1,15,p7), models/ConvAutoEncoder.py:142,171 ------------------------------- */
/* stats [B][ntiles][32][2].  ep_x (optional, y's layout): backward epilogue -- y = conv * swish'(z),
 * z = ep_x*ep_s1[b][c]+ep_t1[b][c]; stats = (sum y, sum y*(ep_x-ep_mean[b][c])*ep_rstd[b][c]) */
int sa_conv1toC(int dtype, const float* x, const float* w, const float* bias, void* y, int B, int L,
                int flip, float* stats, const void* ep_x, const float* ep_s1, const float* ep_t1,
                const float* ep_mean, const float* ep_rstd, void* stream);
int sa_conv1toC_ntiles(int L);
int sa_convCto1(int dtype, const void* x, const float* w, const float* bias, float* y, int B, int L,
                const float* s1, const float* t1, int swish, int flip, void* stream);
int sa_wgrad1C(int dtype, const float* u, const void* v, float* slabs, int B, int L, int chunk,
               int flip, const float* s1, const float* t1, int swish, void* stream);
int sa_wgrad1C_nchunk(int L, int chunk);
/* decoder.8 backward in one launch and one read of v: g [B][L][32] and stats as sa_conv1toC(u, w, flip,
 * ep_x = v, ep_s1 = s1, ...) writes them, slabs [B][sa_wgrad1C_nchunk(L, chunk)][32][15] as sa_wgrad1C(u, v,
 * flip, s1, t1, swish = 1) writes them (same bits).  s1 / t1 / mean / rstd are required; chunk % 512 == 0 */
int sa_bwd1C(int dtype, const float* u, const void* v, const float* w, void* g, float* stats, float* slabs,
             int B, int L, int chunk, int flip, const float* s1, const float* t1, const float* mean,
             const float* rstd, void* stream);
int sa_sum_slabs(const float* slabs, float* dst, int nslab, int n, int accumulate, void* stream);

/* ---- normalisation / activation backward + statistics finalisers (sa_elementwise.hip):
 * nn.InstanceNorm1d(affine), nn.BatchNorm1d (train), x*sigmoid(x), GradReverse
 * (models/ConvAutoEncoder.py:12-28,33-44,119-120,146-169) ---------------------------- */
typedef struct SaEwArgs {
  const void* g; const void* g2; const void* x; void* out;
  const float* s1; const float* t1;
  const float* mean; const float* rstd;
  const float* c1; const float* c2; const float* c3;
  int actbwd, xp_is_act, relu_mask, bstride;
  float* stats;
  int B, L, ntiles;
} SaEwArgs;

int sa_ew_stats(int dtype, int C, const SaEwArgs* a, void* stream);
int sa_ew_apply(int dtype, int C, const SaEwArgs* a, void* stream);
int sa_ew_ntiles(int L);
int sa_sum_partials(const float* slabs, double* dst, int nbatch, int nslab, int n, void* stream);
int sa_sum_rows_d(const double* src, double* dst, int R, int n, void* stream);
int sa_fin_in_fwd(const double* sums, int B, int C, int n, const float* gamma, const float* beta,
                  float eps, float* mean, float* rstd, float* scale, float* shift, void* stream);
/* sums of the BatchNorm finalisers may be R partial rows ([R][groups][2], added in row order).
 * count_dev / n_dev (optional, device fp64 scalar): the element count is read ON THE DEVICE and the
 * host value is ignored -- SyncBatchNorm over ranks with ragged batches all-reduces the per-rank
 * counts beside the sums (torch.nn.SyncBatchNorm exchanges counts the same way) without a host
 * round trip. */
int sa_fin_bn_fwd(const double* sums, int R, int C, double count, const float* gamma, const float* beta,
                  float eps, float momentum, float* run_mean, float* run_var, float* mean,
                  float* rstd, float* scale, float* shift, const double* count_dev, void* stream);
int sa_fin_bn_eval(int C, const float* gamma, const float* beta, float eps, const float* run_mean,
                   const float* run_var, float* mean, float* rstd, float* scale, float* shift,
                   void* stream);
int sa_fin_norm_bwd(const double* sums, const double* lsums, int R, int groups, int C, double n,
                    const float* gamma, const float* mean, const float* rstd, float sign, float* c1,
                    float* c2, float* c3, float* dgamma, float* dbeta, const double* n_dev,
                    void* stream);
int sa_fin_bias(const double* sums, int B, int C, int ncomp, float* db, void* stream);  /* sums [B][C][ncomp] */

/* Bias gradients of several layers at once (the end of a backward stage): for each of the n <= SA_BIAS_MAX
 * records, db[c] = sum over the nbatch x nslab slabs of part[b][s][c][0] (part [nbatch][nslab][C][ncomp] fp32,
 * the per-tile statistics or column-sum slabs of a data-gradient launch) -- what sa_sum_partials + sa_fin_bias do
 * for one layer, same summation order and bits, as TWO launches for all records (rows: fp64 scratch
 * [nbatch][C] per record). */
/* clip_grad_norm_(params, max_norm) of speechbrain's check_gradients (speechbrain_convae_train.py:249) on up to
 * SA_FLATS_MAX flat fp32 gradient buffers (the stage buckets of a backward): total = sqrt(sum g^2),
 * coef = min(1, max_norm / (total + eps)), g *= coef, with torch's clamp(max=1) on non-finite values: a NaN norm
 * gives a NaN coef (every element NaN), an inf norm coef 0 (finite elements 0, infinite ones NaN); g is left
 * untouched only when coef >= 1.  partials: fp64 scratch [SA_FLATS_MAX * 64]; total_norm (optional) receives
 * the norm.  Two launches. */
#define SA_FLATS_MAX 4
typedef struct SaFlat { float* p; long long n; } SaFlat;
typedef struct SaFlats { int n, pad_; SaFlat f[SA_FLATS_MAX]; } SaFlats;
int sa_clip_grads(const SaFlats* f, float max_norm, float eps, double* partials, float* total_norm, void* stream);
/* The arithmetic of torch.optim.Adam(fused=True).step() (fp32, no weight decay / amsgrad / maximize / grad
 * scaler; torch 2.10's fused kernel, same bits) for ntensors tensors in ONE launch (sa_optim.hip).  table
 * (DEVICE memory, ntensors records) names each tensor's parameter, moments, step counter (fp32 scalar, already
 * advanced by the caller) and gradient: bases->f[gbase].p + goff when gbase >= 0 -- a view of a flat gradient
 * bucket, so that buckets reallocated by every backward change an argument, not the table -- else g.  map
 * (DEVICE memory, [nblocks][2] int): block -> (tensor, chunk of SA_ADAM_CHUNK elements).  lr_dev (optional,
 * device fp32 scalar: the capturable optimizer's rate) is read on the device and lr is ignored.
 * sa_adam_record_bytes: sizeof(SaAdamRec), for the binding's layout check. */
#define SA_ADAM_CHUNK 1024
typedef struct SaAdamRec {
  float* p; float* m; float* v; const float* step; const float* g;
  long long goff, n;
  int gbase, pad_;
} SaAdamRec;
int sa_adam_record_bytes(void);
int sa_adam_step(const SaAdamRec* table, int ntensors, const int* map, int nblocks, const SaFlats* bases,
                 const float* lr_dev, double lr, double beta1, double beta2, double eps, void* stream);
#define SA_BIAS_MAX 8
typedef struct SaBiasDesc {
  const float* part; double* rows; float* db;
  int nbatch, nslab, C, ncomp;
} SaBiasDesc;
typedef struct SaBiasMulti { int n, pad_; SaBiasDesc d[SA_BIAS_MAX]; } SaBiasMulti;
int sa_bias_multi(const SaBiasMulti* m, void* stream);

/* ---- classifier head + losses (sa_head.hip): TDNNSexClassifier.forward reshape + pooling
 * (models/ConvAutoEncoder.py:61-66), classify (:47-55), log_softmax (:68); losses at
 * speechbrain_convae_train.py:105-108; utils/cosine_similarity_loss.py:53-56 ---------- */
/* two stages: part [B][nseg][128 channels][128 row residues][2] (nseg = sa_pool_nseg(B)), then
 * sa_pool_gather rotates / sums it into sums [B][128 pooled columns][2] (fp64) */
int sa_pool_fwd(int dtype, const void* r, const float* scale, const float* shift, float* part, int B,
                int L, int nseg, void* stream);
int sa_pool_nseg(int B);
int sa_pool_gather(const float* part, int B, int nseg, int L, double* sums, void* stream);
int sa_pool_fin(const double* sums, int B, int n, const float* noise, float eps, float* pooled,
                float* mean, float* stdraw, void* stream);
/* sa_pool_gather + sa_pool_fin in one launch (same bits).  raw != 0: noise [B][128] is the N(0,1) draw itself
 * and is normalised in the kernel, (g - min g) / max(g - min g) over all B*128 values */
int sa_pool_gather_fin(const float* part, int B, int nseg, int L, const float* noise, int raw, float eps,
                       float* pooled, float* mean, float* stdraw, void* stream);
/* stats (optional, [B][ceil(L/256)][128][2]): partial (sum g, sum g*(r-bn_mean[c])*bn_rstd[c]) of
 * the written gradient, i.e. what sa_ew_stats would compute from g and r in a second pass */
int sa_pool_bwd(int dtype, const void* r, const float* scale, const float* shift,
                const float* dpooled, const float* mean, const float* stdraw, void* g, int B, int L,
                const float* bn_mean, const float* bn_rstd, float* stats, void* stream);
int sa_dense(const float* X, int lda, const float* ps, const float* pt, const float* W, int sbk,
             int sbn, const float* bias, float* Y, int ldy, int M, int N, int K, int relu,
             void* stream);
/* out0 / out1 (either may be NULL): sums[n][0] / sums[n][1] rounded to fp32, written straight into a
 * parameter-gradient tensor (the bias / BatchNorm affine gradients of the FC head) */
int sa_colsums(const float* X, const float* H, const float* hmean, const float* hrstd, int M, int N,
               double* sums, float* out0, float* out1, void* stream);
int sa_bn2d_bwd(const float* G, const float* H, const double* sums, double count, const float* gamma,
                const float* mean, const float* rstd, int relu_mask, int M, int N, float* dH,
                const double* count_dev, void* stream);
int sa_dense_wgrad(const float* dY, const float* X, const float* ps, const float* pt, int M, int N,
                   int K, float* dW, void* stream);
int sa_log_softmax(const float* X, float* Y, int M, int N, void* stream);
int sa_log_softmax_bwd(const float* dY, const float* Y, float* dX, int M, int N, void* stream);
int sa_loss_workspace_bytes(void);
int sa_recon_loss(const float* a, const float* b, long long n, int kind, float* grad, float* loss,
                  void* workspace, void* stream);                /* kind 0 = L1, 1 = MSE */
int sa_cls_losses(const float* logp, const long long* label, int B, int NC, float* out, float* dnll,
                  float* dconf, void* stream);                   /* out = (nll, confusion) */
int sa_cosine_loss(const float* x1, const float* x2, int B, int S, int D, float* rowloss,
                   float* loss, float* dx1, void* stream);
/* The loss tail of the ConvAE train step as two launches.  sa_recon_loss_part: sa_recon_loss without its
 * finaliser; the partial sums stay in the workspace and grad[i] = fl(gscale * g_i), g_i the gradient
 * sa_recon_loss stores.  sa_step_loss (one workgroup): out = (recon, sex, total) with recon / sex the values of
 * sa_recon_loss / sa_cls_losses and total = fl(fl(w_recon*recon) + fl(w_sex*sex)) + 0.0f; dlogp (optional) =
 * dnll * fl(1.0f * w_sex); *nonfinite (optional, device int32) += !isfinite(total). */
int sa_recon_loss_part(const float* a, const float* b, long long n, int kind, float* grad, float gscale,
                       void* workspace, void* stream);
int sa_step_loss(const void* workspace, long long n, const float* logp, const long long* label, int B, int NC,
                 float w_recon, float w_sex, float* out, float* dlogp, int* nonfinite, void* stream);

/* The FC head (classify: Linear(256,128) ReLU BatchNorm Linear(128,64) ReLU BatchNorm Linear(64,2),
 * models/ConvAutoEncoder.py:47-55, + log_softmax :68) as ONE forward and ONE backward launch
 * (sa_head_fused.hip): train mode, local BatchNorm statistics, M <= sa_head_max_rows() rows.
 * sa_head_fwd: pooled [M][256]; w / b: nn.Linear weight / bias; g / be: BatchNorm weight / bias;
 *   rm / rv: running statistics (updated; may be NULL); outputs h1 [M][128], h2 [M][64] (post-ReLU),
 *   f1 [4][128], f2 [4][64] (mean, rstd, scale, shift), logp [M][2].
 * sa_head_bwd: dlogp [M][2] -> every parameter gradient (any may be NULL) and dpooled [M][256].
 * Larger batches, eval mode and SyncBatchNorm use the separate launches above. */
int sa_head_fwd(const float* pooled, const float* w1, const float* b1, const float* g1, const float* be1,
                float* rm1, float* rv1, const float* w2, const float* b2, const float* g2, const float* be2,
                float* rm2, float* rv2, const float* w3, const float* b3, float* h1, float* f1, float* h2,
                float* f2, float* logp, int M, float eps, float momentum, void* stream);
int sa_head_bwd(const float* dlogp, const float* logp, const float* pooled, const float* h1, const float* f1,
                const float* h2, const float* f2, const float* w1, const float* g1, const float* w2,
                const float* g2, const float* w3, float* dw1, float* db1, float* dg1, float* dbe1, float* dw2,
                float* db2, float* dg2, float* dbe2, float* dw3, float* db3, float* dpooled, int M, void* stream);
/* sa_head_bwd over 16 workgroups: each recomputes the dependent chain and writes a slice of d W1, d W2 and
 * dpooled; same arguments, same bits */
int sa_head_bwd_wide(const float* dlogp, const float* logp, const float* pooled, const float* h1, const float* f1,
                     const float* h2, const float* f2, const float* w1, const float* g1, const float* w2,
                     const float* g2, const float* w3, float* dw1, float* db1, float* dg1, float* dbe1, float* dw2,
                     float* db2, float* dg2, float* dbe2, float* dw3, float* db3, float* dpooled, int M,
                     void* stream);
int sa_head_max_rows(void);

/* x-vector gender classifier forward (sa_xvector.hip; models/external_gender_classifiers.py:71-115,144-183;
 * evaluator_inference.yaml:34-48): TDNN block = speechbrain Conv1d (reflect "same" padding) ->
 * LeakyReLU -> BatchNorm1d(eval); StatisticsPooling over time with relative lengths. */
/* wp: sa_pack_weights(SA_BF16X3, ...) image of the Conv1d weight zero-padded to Npad output channels
 * (Npad % 128 == 0; ntaps = K, K = Cin (% 16 == 0), N = Npad, sk = K, sn = Cin*K, st = 1) */
/* mask (optional, [B][T][Cout] bytes): 1 where the LeakyReLU input was positive (for sa_tdnn_bwd_input) */
int sa_tdnn_fwd(const float* x, const void* wp, const float* bias, const float* bn_s, const float* bn_t,
                float* y, int B, int T, int Cin, int Cout, int Npad, int K, int dil, float slope,
                unsigned char* mask, void* stream);
int sa_time_pool(const float* x, const float* lens, const float* noise, int B, int T, int C, float eps,
                 float* out, void* stream);
int sa_leaky_affine(const float* x, const float* s, const float* t, float slope, int M, int C, float* y,
                    void* stream);
/* the same classifier INSIDE the training graph (models/EndToEnd.py:57-61,81: pretrained, frozen):
 * gradient with respect to the input features only.
 * sa_tdnn_bwd_input: dy [B][T][Cy], mask = the forward's LeakyReLU branch mask -> dxe [B][T + dil*(K-1)][Cin],
 *   the data gradient on the range extended by the "same" padding; wp = split-bf16 image of the
 *   Conv1d weight packed as a data-gradient operand (reduction Cred >= Cy, % 16; produced Npad >= Cin,
 *   % 128).  sa_tdnn_fold applies the adjoint of the reflect padding: dxe -> dx [B][T][C].
 * sa_time_pool_bwd: pooled = forward output without the noise offset.  */
int sa_tdnn_bwd_input(const float* dy, const unsigned char* mask, const float* bn_s, const void* wp,
                      float* dxe, int B, int T, int Cy, int Cred, int Cin, int Npad, int K, int dil,
                      float slope, void* stream);
int sa_tdnn_fold(const float* dxe, float* dx, int B, int T, int C, int pad, void* stream);
int sa_time_pool_bwd(const float* x, const float* lens, const float* g, const float* pooled, int B,
                     int T, int C, float eps, float* dx, void* stream);
int sa_leaky_affine_bwd(const float* dy, const float* x, const float* s, float slope, int M, int C,
                        float* dx, void* stream);

/* ---- the x-vector classifier in TRAIN mode (sa_xvector.hip; gender_classifier_train.py):
 * TDNN block z = LeakyReLU(conv_same_reflect(x) + bias), y = BatchNorm1d_train(z) = s*z + t with the
 * statistics over all B*T frames.  No float atomics: every reduction is fixed-order partials.
 * sa_xv_tdnn_fwd_train: x [B][T][Cin] (s_in / t_in: the previous block's BatchNorm affine applied at
 *   staging, both null for block 0), wp = the sa_tdnn_fwd image -> z [B][T][Cout] and fp32 partials
 *   part [B][ntiles][Cout][2] = (sum z, sum z^2) per 128-frame tile (ntiles = sa_xv_tdnn_ntiles(T)).
 * sa_xv_colsums: fp64 partials part [ceil(M/rows_per)][N][2] = (sum v, sum v*h) over row chunks of
 *   G [M][N]; v = G, or with c1..c3 v = (c1*G + c2*H + c3) * (H > 0 ? 1 : slope) also stored to out;
 *   h = H (or v), normalised (h - hmean)*hrstd when hmean != null.  The rows go to sa_fin_bn_fwd,
 *   sa_fin_norm_bwd or sa_fin_bias as R partial rows.
 * sa_xv_tdnn_wgrad: part [nsplit][K][Cout][Cin] = per-split sums over rows r = b*T + t of
 *   dpre[r][co] * x'[b][refl(t + k*dil - pad)][ci] (x' = s_in*x + t_in); rows_per % 32 == 0,
 *   nsplit*rows_per >= B*T, Cin % 4 == 0, Cout % 4 == 0.  sa_xv_wgrad_reduce adds the splits in
 *   order (fp64) into dW [Cout][Cin][K] (the torch Conv1d layout).
 * sa_xv_tdnn_dgrad: dpre [B][T][Cy] -> dxe [B][T + dil*(K-1)][Cin] with the sa_tdnn_bwd_input image;
 *   then sa_tdnn_fold.
 * sa_xv_pool_affine: pooled [B][2C] of y = s*z + t from pz = sa_time_pool(z) (no noise): mean
 *   s*mean_z + t (+ the noise offset), std |s|*std_z + eps.  sa_xv_pool_affine_bwd: g [B][2C] ->
 *   gz (std half times sign(s)) for sa_time_pool_bwd(z, lens, gz, pz), which then yields d loss / d y. */
int sa_xv_tdnn_fwd_train(const float* x, const float* s_in, const float* t_in, const void* wp, const float* bias,
                         float* z, float* part, int B, int T, int Cin, int Cout, int Npad, int K, int dil,
                         float slope, void* stream);
int sa_xv_tdnn_ntiles(int T);
int sa_xv_colsums(const float* G, const float* H, const float* hmean, const float* hrstd, const float* c1,
                  const float* c2, const float* c3, float slope, float* out, int M, int N, int rows_per,
                  double* part, void* stream);
int sa_xv_tdnn_wgrad(const float* dpre, const float* x, const float* s_in, const float* t_in, float* part, int B,
                     int T, int Cin, int Cout, int K, int dil, int nsplit, int rows_per, void* stream);
int sa_xv_wgrad_reduce(const float* part, int nsplit, int K, int Cout, int Cin, float* dW, void* stream);
int sa_xv_tdnn_dgrad(const float* dpre, const void* wp, float* dxe, int B, int T, int Cy, int Cred, int Cin,
                     int Npad, int K, int dil, void* stream);
int sa_xv_pool_affine(const float* pz, const float* s, const float* t, const float* noise, int B, int C,
                      float eps, float* pooled, void* stream);
int sa_xv_pool_affine_bwd(const float* g, const float* s, int B, int C, float* gz, void* stream);

/* ---- model_type fcae (sa_fcae.hip): the reference's FullyConnectedAutoencoder, models/FullyConnected.py:65-104,
 * 118-159, fp32.  feats [B][T][80]; T >= 2; tiles of 64 frames that never cross an utterance.
 *   wb: HOST array of 16 device pointers, the weights then the biases of encoder.0/2/4, decoder.0/2/4,
 *     sex_classifier.initial.0/2 (nn.Linear layout).  hw: HOST array of 16 device pointers of classify:
 *     0.weight 0.bias 1.weight 1.bias 1.running_mean 1.running_var 3.weight 3.bias 5.weight 5.bias 6.weight
 *     6.bias 6.running_mean 6.running_var 7.weight 7.bias.
 *   sa_fc_tiles(T): tiles per utterance.  sa_fc_groups(B, T): workgroups G of the two backward frame passes.
 *   sa_fc_nparam(): floats of one weight-gradient record (the 8 weights, then the 8 biases, in wb order).
 *   sa_fc_nhead(): floats of dhead (d 0.weight 0.bias 1.weight 1.bias 3.weight 3.bias 5.weight 5.bias 6.weight
 *     6.bias 7.weight 7.bias).  sa_fc_max_rows(): largest B of the head launches (larger: -EINVAL).
 * forward:
 *   sa_fc_enc_fwd: h1 [B][T][60], h2 [B][T][40] (post-ReLU), z [B][T][20]; bnpart [B*tiles][20][2] (fp64 sum, sum of
 *     squares per BatchNorm channel; element (t, j) of an utterance is in channel (20 t + j) / T).
 *   sa_fc_bn_fin: bnf [4][20] = mean, rstd, scale, shift; train != 0: batch statistics + running update,
 *     else the running statistics (bnpart unused).
 *   sa_fc_mid_fwd: a1, u [B][T][40] (initial, post-ReLU), d1 [B][T][40], d2 [B][T][60] (decoder, post-ReLU),
 *     recon [B][T][80]; poolpart [B*tiles][2][40] (fp64 sum, sum of squares of u over the tile's frames).
 *   sa_fc_head_fwd: pooled [B][80] = (mean + 1e-5 ((1 - 9) noise + 9) if noise [B][40] != NULL, unbiased std + 1e-5),
 *     pst [B][80] = (mean, std) without either offset, h1 [B][40] (pre-BatchNorm), f1 [4][40], h2 [B][40]
 *     (post-ReLU), h3 [B][20] (pre-BatchNorm), f2 [4][20], logp [B][2].
 * inference:
 *   sa_fc_recon_fwd: recon [B][T][80] = decoder(encoder(feats)) in ONE launch (grid B x tiles): the six layers through
 *     the forward's own tile products, activations in two LDS buffers, nothing else written.  Bit-identical to the
 *     recon of sa_fc_enc_fwd + sa_fc_mid_fwd.  No classifier branch, so none of its limits: any B >= 1
 *     (sa_fc_max_rows does not apply; B <= 65535, the grid's extent), T >= 1.
 * backward:
 *   sa_fc_head_bwd: dlogp [B][2] -> dhead, dpooled [B][80] (the BatchNorm statistics are recomputed from h1 / h3 in
 *     fp64 by the forward's own operations; f1 / f2 are only the forward's record of them).
 *   sa_fc_mid_bwd: d_recon [B][T][80], dpooled -> dzdec (decoder's d z), dzn (d of the BatchNorm output) [B][T][20];
 *     wpart [G][nparam] (decoder.* and initial.* slices), bnbpart [G][20][2] (fp64 sum dy, sum dy * zhat).
 *   sa_fc_bn_bwd_fin: coef [3][20] of d z = c1 dzn + c2 z + c3 (GradReverse folded in), dgamma, dbeta [20].
 *   sa_fc_enc_bwd: wpart (encoder.* slices).  No gradient to feats.
 *   sa_fc_wreduce: grads [nparam] = the G records added in order (fp64). */
int sa_fc_tiles(int T);
int sa_fc_groups(int B, int T);
int sa_fc_nparam(void);
int sa_fc_nhead(void);
int sa_fc_max_rows(void);
int sa_fc_enc_fwd(const float* feats, const void* const* wb, float* h1, float* h2, float* z, double* bnpart,
                  int B, int T, void* stream);
int sa_fc_bn_fin(const double* bnpart, int npart, const float* gamma, const float* beta, float* run_mean,
                 float* run_var, float* bnf, int B, int T, int train, float eps, float momentum, void* stream);
int sa_fc_mid_fwd(const float* z, const float* bnf, const void* const* wb, float* a1, float* u, float* d1,
                  float* d2, float* recon, double* poolpart, int B, int T, void* stream);
int sa_fc_recon_fwd(const float* feats, const void* const* wb, float* recon, int B, int T, void* stream);
int sa_fc_head_fwd(const double* poolpart, const float* noise, const void* const* hw, float* pooled, float* pst,
                   float* h1, float* f1, float* h2, float* h3, float* f2, float* logp, int B, int T, int train,
                   float eps, float momentum, void* stream);
int sa_fc_head_bwd(const float* dlogp, const float* logp, const float* pooled, const float* h1,
                   const float* h2, const float* h3, const void* const* hw, float* dhead,
                   float* dpooled, int B, int train, float eps, void* stream);
int sa_fc_mid_bwd(const float* d_recon, const float* dpooled, const float* pst, const float* z, const float* bnf,
                  const float* a1, const float* u, const float* d1, const float* d2, const void* const* wb,
                  float* dzn, float* dzdec, float* wpart, double* bnbpart, int B, int T, void* stream);
int sa_fc_bn_bwd_fin(const double* bnbpart, int npart, const float* gamma, const float* bnf, float* coef,
                     float* dgamma, float* dbeta, int B, int T, int train, void* stream);
int sa_fc_enc_bwd(const float* feats, const float* h1, const float* h2, const float* z, const float* dzn,
                  const float* dzdec, const float* coef, const void* const* wb, float* wpart, int B, int T,
                  void* stream);
int sa_fc_wreduce(const float* wpart, int G, float* grads, void* stream);

/* ---- k-NN mutual information (sa_mi.hip): utils/ClusterMI.py:88-121,
 * utils/GroupSamplingMI.py:49-61, utils/mi_loss.py:14-17 ------------------------------ */
int sa_cluster_mi(const float* X, const long long* y, const long long* idx, int iters, int n, int D,
                  int ncls, int k, float* mi, void* stream);

/* ---- feature front-end (sa_fbank.hip): speechbrain Fbank + InputNormalization at
 * speechbrain_convae_train.py:58-63,82-87 (convae.yaml:93-95,269-271,289-292) --------- */
/* dft / mel: bf16 fragment-major operand images built once by the host (layout in sa_fbank.hip;
 * speech-anonymization_amd/features.py builds them), sa_fbank_table_elems(0 | 1) elements each */
int sa_fbank(const float* wav, int B, int N, const float* window, const void* dft,
             const void* mel, float* feats, float* tilemax, void* stream);
int sa_fbank_table_elems(int which);
int sa_fbank_ntiles(int T);
int sa_fbank_scratch_bytes(int B);
int sa_fbank_normalize(const float* feats, const float* tilemax, int B, int T, int Tp,
                       const float* lens, float top_db, int batch_max, int update, int epoch,
                       int update_until_epoch, float* state, float* scratch, float* out,
                       void* stream);
/* two successive sa_fbank_normalize calls on the same features (the train step's input and target) from
 * one read of them: out1 / out2 and the final state have the bits of the two calls.  snap: 160 floats of
 * scratch.  out2 may be NULL when neither update moves mean / std (update == 0, or epoch >=
 * update_until_epoch with count > 0): both results are then out1 */
int sa_fbank_normalize_pair(const float* feats, const float* tilemax, int B, int T, int Tp,
                            const float* lens, float top_db, int batch_max, int update, int epoch,
                            int update_until_epoch, float* state, float* scratch, float* snap,
                            float* out1, float* out2, void* stream);

/* ---- waveform augmentation of the gender-classifier recipes (sa_augment.hip): additive noise
 * rows, speed perturbation, frequency drop and chunk drop of speechbrain's env_corrupt / TimeDomainSpecAugment,
 * restated.  wav, noise [B][L] fp32; every random draw but the noise is made by the host (augment.draw_plan).
 *   sa_wav_abs_sums: sums [2][B] fp64 = per-row sum |x| of wav, then of noise (noise NULL: the first B only);
 *     fp64 partials added in a fixed order, no atomics.
 *   sa_noise_scales: scales [B][2] = (1 - f, f amp_c / (amp_n + 1e-14)), amp = sum / (lens L),
 *     f = 1 / (10^(snr / 20) + 1); lens, snr [B] fp32 on the device; fp64 arithmetic, rounded once.
 *   sa_wav_augment: out [R][Lp], R = B (rows as they are) or 2 B (row B + b = scales[b][0] wav[b] + scales[b][1]
 *     noise[b], formed at staging) -> resampled by the S_out x W table (output q S_out + i = sum_j w[i][j]
 *     x[q S_in + first[i] + j], zeros outside [0, L)) -> 101-tap filter y[n] = sum_j h[j] r[n + j - 50], zeros
 *     outside [0, Lp) -> the row's intervals zeroed.  ONE launch, grid (tiles of sa_wav_augment_tile() samples, R).
 *     plan: 32-bit words in device memory: first [S_out] int, w [S_out][W] float, h [101] float, chunks
 *     [R][1 + 2 sa_wav_augment_max_chunks()] int (count, then start, end pairs; end exclusive).  first_min /
 *     first_max: the extremes of first[].  -EINVAL: R not B or 2 B, R > 65535, S_out > 128, W > 32, S_out W > 2048,
 *     a ratio S_in / S_out whose tile span exceeds the staging buffer (speeds under ~72 %). */
int sa_wav_augment_tile(void);
int sa_wav_augment_max_chunks(void);
int sa_wav_abs_sums(const float* wav, const float* noise, int B, int L, double* sums, void* stream);
int sa_noise_scales(const double* sums, const float* lens, const float* snr, int B, int L, float* scales,
                    void* stream);
int sa_wav_augment(const float* wav, const float* noise, const float* scales, const void* plan, int B, int L, int R,
                   int Lp, int S_in, int S_out, int W, int first_min, int first_max, float* out, void* stream);

/* ---- SpecAugment of the ConvAE train step's input features (sa_specaug.hip): bicubic time warp,
 * frequency masks and time masks of speechbrain's lobes.augment.SpecAugment, restated.  x, out [B][T][F] fp32, 16-byte
 * aligned, x != out; every random draw is made by the host (specaug.draw_plan).
 *   plan: 32-bit words in device memory: header [8] (flags: bit 0 = fill with zero; B; T; F; 0 ...), rows [T][8]
 *     (base, lo, hi, 0 as int, then four float weights: out row o = sum_k w[k] x[clamp(base - 1 + k, lo, hi)]),
 *     freq [B][8][2] and time [B][8][2] (pos, len; len 0 = unused), n_fm [B] (frequency-masked cells per utterance).
 *   sa_specaug_warp_sums: out = the warped rows; part [ceil(T / 32) * B][2] fp64 = per workgroup the sum of its
 *     values and of those in frequency-masked columns.  Grid (tiles of 32 frames, B); no atomics.
 *   sa_specaug_finalize: vals [2] = (val_f, val_t): val_f = S / N, val_t = (S - S_fm + n_fm val_f) / N, N = B T F,
 *     fp64 sums in a fixed order, each rounded once to fp32; both 0 with the zero flag.
 *   sa_specaug_fill: out's time-masked rows = val_t, elsewhere its frequency-masked columns = val_f.
 *   -EINVAL: B < 1 or > 65535, T < 1, F no multiple of 4 or > 128, a NULL or misaligned pointer, x == out. */
int sa_specaug_warp_sums(const float* x, const void* plan, int B, int T, int F, float* out, double* part,
                         void* stream);
int sa_specaug_finalize(const double* part, const void* plan, int B, int T, int F, float* vals, void* stream);
int sa_specaug_fill(const void* plan, const float* vals, int B, int T, int F, float* out, void* stream);

/* ---- Griffin-Lim inversion of the features (sa_vocoder.hip): normalised log-Mel frames back to
 * a waveform.  n_fft 400, hop 160, 201 bins, the front end's periodic Hamming window, center=True with zero padding:
 * T frames <-> N = (T - 1) 160 samples.  Complex spectra are [B][T][201] interleaved (re, im) fp32.  window [400];
 * twiddle [800] = cos then sin(2 pi i / 400), i = 0..399 (fp64 rounded once; read at (k j) mod 400).
 *   sa_mel_to_mag: S [B][T][201] = sqrt(max(0, sum_m p_m M[m][k])), p_m = 10^((x[b][t][m] std[m] + mean[m]) / 10);
 *     x [B][Tf][80], frames t >= T of it are not read; M [80][201] the filterbank's pseudo-inverse.
 *   sa_gl_istft: y [B][N] = torch.istft(C, center=True, length=N): windowed inverse real DFTs (the imaginary parts of
 *     bins 0 and 200 do not enter), overlap-added by gathering and divided by the envelope sum_t w^2.
 *   sa_gl_project: R = STFT(y) (zero padding, center=True); A = R - m Tprev; C_new = S A / (|A| + 1e-16), the update
 *     in fp64 from the fp32 values, rounded once; R is stored too (the next call's Tprev; C_new, R != Tprev).
 *   sa_gl_tile: hop blocks of output (sa_gl_istft) and frames (sa_gl_project) per workgroup.
 *   Grids are (tiles, B).  -EINVAL: a NULL pointer, B < 1 or > 65535 (grid.y), T < 2 (sa_mel_to_mag: T < 1) or
 *     T > 2^23 (160 T + 400 stays an int), T > Tf. */
int sa_gl_tile(void);
int sa_mel_to_mag(const float* x, const float* mean, const float* stdv, const float* M, int B, int T, int Tf,
                  float* S, void* stream);
int sa_gl_istft(const void* C, const float* window, const float* twiddle, int B, int T, float* y, void* stream);
int sa_gl_project(const float* y, const float* S, const void* Tprev, float momentum_ratio, const float* window,
                  const float* twiddle, int B, int T, void* C_new, void* R, void* stream);

/* ---- pitch normalisation (sa_pitch.hip): an F0 tracker and the passes that, around
 * sa_gl_istft / sa_gl_project, scale a waveform's pitch by a per-utterance ratio.  16 kHz, hop 160.
 *   sa_yin_dim(which): 0 sample rate 16000, 1 hop 160, 2 W 400, 3 tau_min 40, 4 tau_max 266, 5 L = W + tau_max
 *     666, 6 frames per workgroup of sa_yin_f0, 7 outputs per workgroup of sa_pitch_resample; else -EINVAL.
 *   sa_yin_f0: wav [B][N] -> f0 [B][T] in Hz (0: unvoiced), T = N / 160 + 1.  Frame t reads x[j] =
 *     wav[160 t - 333 + j], j < L, zeros outside [0, N); d(tau) = sum_{j < W} (x[j] - x[j + tau])^2 summed as
 *     written; d'(tau) = d(tau) tau / sum_{i <= tau} d(i) (1 where the sum is 0; d'(0) = 1); the pick is the
 *     smallest tau in [tau_min, tau_max - 1] with d' < threshold, d'(tau) <= d'(tau - 1), d'(tau) < d'(tau + 1),
 *     refined by the parabola through its neighbours (fp64 from the fp32 d', rounded once); no pick: 0.
 *     dprime: NULL, or [B][T][tau_max + 1] to receive d' (tests).
 *   sa_pitch_ratio: over the first round(lens_b N) / 160 + 1 (at most T) frames of row b: voiced_b = the count
 *     of f0 > 0, mean_b their mean (fp64, fixed order; 0 without any), ratio_b = clamp(target / mean_b, r_min,
 *     r_max) if voiced_b >= min_voiced, else 1.
 *   sa_pitch_stretch_mag: R complex [B][T][201] -> S [B][Tout][201]: for t' < T'_b = ceil((T - 1) r_b) + 1,
 *     (1 - a) |R[i]| + a |R[i + 1]| at pos = min(t' / r_b, T - 1) (fp64), i = min(floor(pos), T - 2), a = pos - i;
 *     0 from T'_b on.  Tout is the caller's max_b T'_b (a smaller one truncates).
 *   sa_pitch_resample: y [B][Nin] -> out [B][Nout]: out[n] = sum_i y[i] h(n r_b - i) for n < n_valid[b], else 0;
 *     h(u) = c sinc(c u) (0.5 + 0.5 cos(pi u / H)) on |u| < H, c = min(1, 1 / r_b), H = 16 / c (at most 64 taps;
 *     position and weights in fp64, weights rounded once, fp32 accumulation).  Row b's input ends at
 *     min(Nin, 160 ceil(ceil(Nout / 160) r_b)) samples -- (T'_b - 1) 160 of a waveform of Nout samples.
 *   The ratios are read on the device: a value outside [0.5, 2] is taken as the nearer bound, a NaN as 1.
 *   -EINVAL: a NULL pointer (dprime may be NULL), B < 1 or > 65535 (grid.y), N, Nin < 1 or > 2^30, Nout < 1 or
 *     > 2^29, T < 1 (stretch: < 2) or T, Tout > 2^23, target <= 0, r_min < 0.5, r_max > 2, r_min > r_max. */
int sa_yin_dim(int which);
int sa_yin_f0(const float* wav, int B, int N, float threshold, float* f0, float* dprime, void* stream);
int sa_pitch_ratio(const float* f0, const float* lens, int B, int T, int N, float target, float r_min, float r_max,
                   int min_voiced, float* ratio, float* mean, int* voiced, void* stream);
int sa_pitch_stretch_mag(const void* R, const float* ratio, int B, int T, int Tout, float* S, void* stream);
int sa_pitch_resample(const float* y, const float* ratio, const int* n_valid, int B, int Nin, int Nout, float* out,
                      void* stream);

/* ---- spectral envelope and formant warp (sa_envelope.hip): the source-filter split of the
 * pitch path.  n_fft 400, 201 bins, w_k = 2 pi k / 400.  For every frame of magnitudes S [B][T][201] >= 0:
 *     L[k] = ln(max(S[k], floor_rel max_k S, 1e-10));
 *     c_n = (1 / 400) [L_0 + (-1)^n L_200 + 2 sum_{k = 1..199} L_k cos(2 pi n k / 400)], n = 0..n_c (the real
 *       cepstrum of the even extension);
 *     E(w) = c_0 + 2 sum_{n = 1..n_c} c_n cos(n w);
 *     g[k] = clamp(E(min(pi, q_b w_k)) - E(w_k), +-max_gain_ln);  out[k] = S[k] exp(g[k]).
 *   An all-zero frame gives zeros; a row with q_b == 1 is copied bit for bit.  q [B] is read on the device: a
 *   value outside [0.25, 4] is taken as the nearer bound, a NaN as 1.  env: NULL, or [B][T][201] to receive
 *   E(w_k) (tests).  out != S.
 *   sa_env_dim(which): 0 n_fft 400, 1 bins 201, 2 frames per workgroup, 3 the largest n_c 64, 4 threads per
 *     workgroup; else -EINVAL.
 *   -EINVAL: a NULL pointer (env may be NULL), B < 1 or > 65535 (grid.y), T < 1 or > 2^23, n_c outside 1..64,
 *     floor_rel outside (0, 1), max_gain_ln <= 0. */
int sa_env_dim(int which);
int sa_env_warp(const float* S, const float* q, int B, int T, int n_c, float floor_rel, float max_gain_ln,
                float* out, float* env, void* stream);

/* ---- McAdams-coefficient anonymisation (sa_mcadams.hip; mcadams.py): VoicePrivacy's
 * signal-processing baseline.  wav [B][N] fp32, alpha [B] fp32, n_valid [B] int32 -> out [B][N] fp32, out != wav.
 * Frames of W = 320 at hop H = 160 under the periodic sqrt-Hann window w, T = (N + 159) / 160 + 1 of them, frame t
 * over the samples [160 t - 160, 160 t + 160); a sample outside [0, n_valid_b) reads as 0.  Per frame, in fp64:
 *     f = w x;  r_k = sum_j f[j] f[j + k], k = 0..20;  r_0 < 1e-10: silent (status 1), rec = f;  r_0 *= 1 + 1e-9;
 *     a[0..20] by Levinson-Durbin; some |k_i| >= 1 or a prediction error <= 0: fallback (status 2), rec = f;
 *     the 20 roots z of a by Aberth-Ehrlich from 0.9 exp(2 pi i (j + 0.25) / 20), stopped when the largest
 *       correction is under 1e-14, given up (fallback) after 64 iterations;  a root is real when
 *       |Im z| <= 1e-6 |z|, kept when Im z > 1e-6 |z|, dropped otherwise;  2 kept + real != 20: fallback;
 *     a' = prod_real (1 - Re z x) prod_kept (1 - 2 |z| cos(phi^alpha) x + |z|^2 x^2), phi = arg z;
 *     res = FIR(a) f, rec = IIR(1 / a') res, both from zero history;  the frame stored is fp32(rec w).
 *   y[n] = F_t0[n - 160 t0 + 160] + F_{t0 + 1}[n - 160 t0], t0 = n / 160 (fp32);  out[n] = fp32(g_b y[n]) for
 *   n < n_valid_b and 0 from there on;  level != 0: g_b = sqrt(sum x^2 / sum y^2) over n < n_valid_b (fp64, a fixed
 *   order; 1 when either sum is 0), else 1.  alpha is read on the device: a value outside [0.25, 2] is taken as the
 *   nearer bound, a NaN as 1; a row whose alpha is 1 is copied bit for bit below n_valid_b (gain 1, status 0).
 *   n_valid_b is clamped to [0, N].  The same bits on every run.
 *   ws: the caller's, 4 B T 320 + 8 (2 B ceil(N / C) + B) bytes, 8-byte aligned, C = sa_mcadams_dim(6); its
 *     contents mean nothing between calls.  status: NULL, or int32 [B][T].  gain: NULL, or fp32 [B].
 *   sa_mcadams_dim(which): 0 W 320, 1 H 160, 2 P 20, 3 frames per workgroup, 4 threads per workgroup, 5 the largest
 *     iteration count 64, 6 samples per block of the level sums; else -EINVAL.
 *   -EINVAL, before any launch: a NULL pointer (status and gain may be NULL), B < 1 or > 65535 (grid.y), N < 1 or
 *     > 2^30, T > 2^23. */
int sa_mcadams_dim(int which);
int sa_mcadams(const float* wav, const float* alpha, const int* n_valid, int B, int N, int level, float* out,
               void* ws, int* status, float* gain, void* stream);

/* ---- STOI / ESTOI intelligibility scoring (sa_stoi.hip; ops.stoi): Taal et al. 2011 and
 * Jensen & Taal 2016 on the original and the processed waveform, no pretrained model.  ref, deg [B][N] fp32 at
 * 16 kHz, n_valid [B] int32 (clamped to [0, N]; a sample at or beyond n_valid_b reads as 0 in both signals) ->
 * stoi, estoi [B] fp32, frames, segments [B] int32.  In exact terms (the kernels evaluate it in fp64), eps = 2^-52:
 *   (1) to 10 kHz: n10 = (5 n_valid + 7) / 8;  x10[m] = sum_n x[n] h[8 m - 5 n] over |8 m - 5 n| <= 80 (at most 33
 *       taps, ascending n);  h[k] = (5/8) sinc(k/8) I0(5 sqrt(1 - (k/80)^2)) / I0(5), k = -80..80: taps[k + 80],
 *       161 doubles in device memory, built by the caller.  deg the same way.
 *   (2) silent frames, decided on ref:  w[j] = 0.5 - 0.5 cos(2 pi (j + 1) / 257), j = 0..255;
 *       F = (n10 - 256) / 128 + 1 frames when n10 >= 256, else 0, frame t over [128 t, 128 t + 256);
 *       e_t = sum_j (w[j] x10[128 t + j])^2;  kept when e_t > 1e-4 max_t e_t (strict; 40 dB in the power domain);
 *       K kept frames t_0 < ... < t_{K-1}.
 *   (3) xs[n] = sum_{i : 128 i <= n < 128 i + 256} w[n - 128 i] x10[128 t_i + n - 128 i], n < 128 (K + 1); the same
 *       t_i for deg.
 *   (4) frame m = 0..K-1 of xs times w, zero-padded to 512, P[m][k] = |DFT|^2;
 *       X[j][m] = sqrt(sum_{lo_j <= k < hi_j} P[m][k]) over the 15 third-octave bands (centres 150 2^(j/3) Hz, edges
 *       at -+1/6 octave, rounded to the nearest bin): (7,9) (9,11) (11,14) (14,17) (17,22) (22,27) (27,34) (34,43)
 *       (43,55) (55,69) (69,87) (87,109) (109,138) (138,174) (174,219).  Y from deg.
 *   (5) segments m = 30..K over the frames m - 30..m - 1: S = K - 29 when K >= 30, else 0.
 *       STOI, per band and segment: alpha = |x| / (|y| + eps);  y' = min(alpha y, (1 + 10^0.75) x);
 *         x~ = (x - mean x) / (|x - mean x| + eps), y~ the same of y';  d = sum x~ y~;  stoi = the mean of d over the
 *         15 S pairs.
 *       ESTOI, per segment on the 15 x 30 matrices: rows made zero-mean and unit-norm along time, then columns
 *         along the bands, every norm + eps;  d_m = (1/30) sum of the element-wise product;  estoi = mean_m d_m.
 *   A row with S = 0 (fewer than 30 kept frames, an all-zero ref, n_valid = 0) gets stoi = estoi = 0, segments = 0.
 *   estoi, frames and segments may be NULL.  No atomics, every sum in a fixed order: the same bits on every run.
 *   ws: the caller's, 8 B (2 M + 33 F) + 4 B (F + 2) bytes, 8-byte aligned, with M = (5 N + 7) / 8 and
 *     F = (M - sa_stoi_dim(1)) / sa_stoi_dim(2) + 1 when M >= sa_stoi_dim(1), else 1; its contents mean nothing
 *     between calls.
 *   sa_stoi_dim(which): 0 the inner rate 10000, 1 the frame 256, 2 the hop 128, 3 the transform 512, 4 bands 15,
 *     5 frames per segment 30, 6 taps 161, 7 compacted frames per workgroup of the band kernel, 8 segments per
 *     workgroup, 9 threads per workgroup; else -EINVAL.
 *   -EINVAL, before any launch: a NULL pointer (estoi, frames and segments may be NULL), B < 1 or > 65535 (grid.y),
 *     N < 1 or > 2^24. */
int sa_stoi_dim(int which);
int sa_stoi(const float* ref, const float* deg, const int* n_valid, int B, int N, const double* taps,
            float* stoi, float* estoi, int* frames, int* segments, void* ws, void* stream);

/* ---- phase-vocoder resynthesis (sa_phasevoc.hip; ops.pv_synth): the stretch of
 * sa_pitch_stretch_mag with the input's phases carried through it.  R [B][T][201] complex64 (the STFT of the padded
 * waveform), ratio [B] fp32, read on the device as sa_pitch_stretch_mag reads it (outside [0.5, 2]: the nearer bound,
 * NaN: 1) -> C [B][Tout][201] complex64, C != R.  Phases in turns (1 turn = 2 pi), fp64:
 *     theta[i][k] = atan2(im, re) / (2 pi) of R[i][k], formed in fp64 from the fp32 values (IEEE signed zeros;
 *       (0, 0) -> 0);
 *     T'_b, pos, i_s = min(floor(pos), T - 2) and a_s of output frame s exactly as in sa_pitch_stretch_mag;
 *     phi'[0][k] = theta[0][k] mod 1;  phi'[t' + 1][k] = (phi'[t'][k] + theta[i_t' + 1][k] - theta[i_t'][k]) mod 1
 *       for t' + 1 < T'_b (x mod 1 = x - floor(x): the accumulator never leaves [0, 1]);
 *     C[t'][k] = S'[t'][k] (cospi(2 phi'), sinpi(2 phi')), formed in fp64, each component rounded once to fp32;
 *       0 for t' >= T'_b.
 *   S: the magnitudes S' [B][Tout][201] fp32 (e.g. sa_env_warp's output), or NULL: S' = (1 - a) |R_i| + a |R_{i+1}|,
 *     bit for bit what sa_pitch_stretch_mag writes.  phase: NULL, or fp64 [B][Tout][201] to receive phi' (0 for
 *     t' >= T'_b; tests).  At ratio 1 the sum telescopes: C = R S' / |R|.
 *   The sum runs as a chunked scan of three launches (chunk totals, chunk offsets, synthesis): sums of a different
 *   grouping than the recurrence above, in a fixed order -- the same bits on every run, within (Tout + 8) 2^-50
 *   turns of the recurrence.  No atomics, and no workgroup waits on another.
 *   ws: the caller's, sa_pv_workspace_bytes(B, Tout) = 8 B ceil(Tout / Tc) 201 bytes, 8-byte aligned, Tc =
 *     sa_pv_dim(3); its contents mean nothing between calls.  (-EINVAL for a B or Tout sa_pv_synth refuses.)
 *   sa_pv_dim(which): 0 n_fft 400, 1 hop 160, 2 bins 201, 3 output frames per chunk Tc, 4 threads per workgroup;
 *     else -EINVAL.
 *   -EINVAL, before any launch: a NULL pointer (S and phase may be NULL), B < 1 or > 65535 (grid.y), T < 2 or
 *     > 2^23, Tout < 1 or > 2^23. */
int sa_pv_dim(int which);
long long sa_pv_workspace_bytes(int B, int Tout);
int sa_pv_synth(const void* R, const float* S, const float* ratio, int B, int T, int Tout, void* C, double* phase,
                void* ws, void* stream);

/* ---- F0-contour pitch modification (sa_contour.hip, with one variant each in sa_phasevoc.hip and sa_envelope.hip;
 * DESIGN section 20): a ratio per frame on the phase-vocoder path, so that the output contour is target + gamma (f0
 * - mean).  HOP 160.  Two tables per row carry it, both on the device:
 *     rho_q [B][T] int32: the ratio of frame t in units of 2^-16, in [2^15, 2^17];
 *     Q [B][T] int64: the time map, Q[0] = 0, Q[t + 1] = Q[t] + w[t], w[t] = rho_q[t] + rho_q[t + 1] (the mean ratio
 *       of hop interval t in units of 2^-17);  T'_b = ((Q[T - 1] + 2^17 - 1) >> 17) + 1 output frames.
 *   Every kernel clamps what it reads from them (rho_q to [2^15, 2^17], w to [2^16, 2^18], Q[T - 1] to [0, (T - 1)
 *   2^18]) and every index it derives (i to [0, T - 2], a to [0, 1]).
 *   sa_pitch_contour: f0 [B][T] (sa_yin_f0 of the padded waveform, T >= 2) -> rho_q, Q, Tq [B] = T'_b, and mean [B],
 *     voiced [B] exactly as sa_pitch_ratio forms them (the first round(lens_b N) / 160 + 1 frames count; a frame
 *     beyond them is not voiced whatever it holds).  A row with voiced_b < min_voiced, or with no voiced frame, gets
 *     rho_q = 2^16 throughout.  Otherwise, in fp64, for every t < T:
 *       f^[t] = f0[t] on a voiced frame, else f0[l] + (f0[n] - f0[l]) (t - l) / (n - l) between the last voiced
 *         frame l before t and the first one n after it, or the value of the one that exists;
 *       f~[t] = sum_{|j| <= s} (s + 1 - |j|) f^[clamp(t + j, 0, T - 1)] / (s + 1)^2, j ascending, s = smooth;
 *       rho_q[t] = rint(2^16 clamp(max(60, target + gamma (f~[t] - mean_b)) / f~[t], r_min, r_max)).
 *     One workgroup per row walks T in passes of sa_contour_dim(0) frames: l and n by a max- and a min-scan of the
 *     voiced indices, Q by an int64 scan, each with a carry between the passes.
 *   sa_pv_synth_map: sa_pv_synth with the stretch positions of the time map.  Output frame t' < T'_b, X = t' 2^17:
 *     X >= Q[T - 1]: i = T - 2, a = 1; else i the largest index <= T - 2 with Q[i] <= X and a = (double)(X - Q[i]) /
 *     (double)w[i] rounded once to fp32.  Phases and synthesis as in sa_pv_synth; the magnitude is (1 - a) M[i] +
 *     a M[i + 1] with M [B][T][201] fp32 ON THE INPUT GRID, or |R| when M is NULL.  At a constant rho_q = r 2^16 it
 *     writes sa_pv_synth's bits at ratio r.  ws: sa_pv_workspace_bytes(B, Tout).
 *   sa_env_warp_frames: sa_env_warp with q [B][T], one factor per frame; for q constant along t, the same bits.
 *   sa_pitch_resample_map: y [B][Nin] -> out [B][Nout].  For n < n_valid[b], t = min(n / 160, T - 2), u = n - 160 t:
 *     Z = 160 Q[t] + w[t] u, ip = Z >> 17, fr = (Z mod 2^17) / 2^17, r = w[t] / 2^17, c = min(1, 1 / r), H = 16 / c;
 *     out[n] = sum_i y[i] h(ip - i + fr) with sa_pitch_resample's h (weights in fp64, rounded once, fp32
 *     accumulation in the order of i); i outside [0, min(Nin, (T'_b - 1) 160)) contributes nothing; 0 for
 *     n >= n_valid[b].
 *   sa_contour_dim(which): 0 frames per pass of sa_pitch_contour, 1 the largest smooth 8, 2 hop 160, 3 fraction bits
 *     of rho_q 16, 4 of Q 17, 5 outputs per workgroup of sa_pitch_resample_map, 6 samples it stages; else -EINVAL.
 *     (sa_pv_dim and sa_env_dim hold for the two variants.)
 *   -EINVAL, before any launch: a NULL pointer (M, phase and env may be NULL), B < 1 or > 65535, T < 2 (sa_env_warp_
 *     frames: < 1) or > 2^23, Tout < 1 or > 2^23, N, Nin < 1 or > 2^30, Nout < 1 or > 2^29, target <= 0, gamma
 *     outside [0, 2], smooth outside 0..8, r_min < 0.5, r_max > 2, r_min > r_max, and sa_env_warp's conditions. */
int sa_contour_dim(int which);
int sa_pitch_contour(const float* f0, const float* lens, int B, int T, int N, float target, float gamma, int smooth,
                     float r_min, float r_max, int min_voiced, int* rho_q, long long* Q, int* Tq, float* mean,
                     int* voiced, void* stream);
int sa_pv_synth_map(const void* R, const float* M, const int* rho_q, const long long* Q, int B, int T, int Tout,
                    void* C, double* phase, void* ws, void* stream);
int sa_env_warp_frames(const float* S, const float* q, int B, int T, int n_c, float floor_rel, float max_gain_ln,
                       float* out, float* env, void* stream);
int sa_pitch_resample_map(const float* y, const int* rho_q, const long long* Q, const int* n_valid, int B, int Nin,
                          int Nout, int T, float* out, void* stream);

/* ---- Viterbi F0 tracking (sa_f0track.hip; ops.f0_candidates, ops.f0_viterbi): a path through the
 * dips of every frame's d' in place of YIN's first dip under the threshold.  dprime [B][T][267] fp32 is what
 * sa_yin_f0 writes; tau_min = 40, tau_max = 266 (sa_yin_dim); K = 8 candidates per frame; states 0..7 are the
 * candidates in ascending lag, state 8 is unvoiced.  Every cost is an integer in units of 2^-16.
 *   sa_f0_candidates: a lag tau in [tau_min, tau_max - 1] is a dip when d'(tau) <= d'(tau - 1) and d'(tau) <
 *     d'(tau + 1); its cost is q = rint(clamp(d'(tau), 0, 1) 2^16).  The K dips of smallest (q, tau), in that
 *     lexicographic order, go to cand_tau, cand_q [B][T][K] int32 in ascending tau; unused slots hold tau = -1, q = 0.
 *   sa_f0_viterbi, per row b over its first F_b = min(T, round(lens_b N) / 160 + 1) frames (formed as sa_pitch_ratio
 *     forms it):  the weights voicing_cost v, switch_cost s, jump_cost j (per octave) and lag_bias beta (per octave)
 *     become ints once, on the host: w_q = (int)lrint(w 2^16).  LOG = log_q, int32 [tau_max + 1], the caller's:
 *     rint(log2(max(tau, 1)) 2^16).
 *       local cost   l(t, i) = q + ((beta_q (LOG[tau] - LOG[tau_min])) >> 16) for a present candidate, l(t, 8) = v_q;
 *                    an absent candidate (tau < 0) is not a state;
 *       transition   0 unvoiced -> unvoiced;  s_q between voiced and unvoiced, either way;
 *                    (j_q |LOG[tau_a] - LOG[tau_s]|) >> 16 between two candidates;
 *       delta_0(s) = l(0, s);  delta_t(s) = l(t, s) + min_a (delta_{t-1}(a) + trans(a, s)), psi_t(s) the argmin;
 *       ties go to the smaller state index, at every step and in the final argmin over delta at F_b - 1.
 *     int64 sums throughout.  psi: the caller's workspace, uint8 [B][T][K + 1]; its contents mean nothing between
 *     calls.  path [B][T] int32: the candidate index after the backtrace, -1 for unvoiced and for t >= F_b.
 *     f0 [B][T] fp32: 16000 / (tau + off) of the chosen lag with sa_yin_f0's parabola (fp64 from the fp32 d', den > 0
 *     else off = 0, rounded once) -- a frame on which both trackers choose the same lag carries the same bits; 0 for
 *     unvoiced frames and for t >= F_b.
 *   What the kernels read from device memory is clamped before it becomes an index: cand_tau to -1 or [tau_min,
 *   tau_max - 1], cand_q to [0, 2^16], lens as sa_pitch_ratio does, every index into LOG to [0, tau_max].
 *   One wave per frame (candidates) and per row (decode); no atomics: the same bits on every run.
 *   sa_f0v_dim(which): 0 K = 8, 1 states 9, 2 frames per workgroup of sa_f0_candidates, 3 frames per staged chunk of
 *     sa_f0_viterbi, 4 cost fraction bits 16; else -EINVAL.
 *   -EINVAL, before any launch: a NULL pointer, B < 1 or > 65535, T < 1 or > 2^23, N < 1 or > 2^30, a weight that is
 *     NaN or outside [0, 4]. */
int sa_f0v_dim(int which);
int sa_f0_candidates(const float* dprime, int B, int T, int* cand_tau, int* cand_q, void* stream);
int sa_f0_viterbi(const float* dprime, const int* cand_tau, const int* cand_q, const float* lens, const int* log_q,
                  int B, int T, int N, float voicing_cost, float switch_cost, float jump_cost, float lag_bias,
                  unsigned char* psi, int* path, float* f0, void* stream);

/* ---- pitch-correlation scoring (sa_prosody.hip; ops.f0_compare): how much of one F0 track's
 * movement is found in another.  f0_ref, f0_deg [B][T] fp32 in Hz, 0 or less meaning unvoiced (any two tracks of
 * sa_yin_f0 or sa_f0_viterbi); frames [B] int32, clamped where it is read to F_b in [0, T]; max_lag Lg in 0..32
 * frames; min_common m >= 2.  Everything in fp64 on the fp32 inputs:
 *   v_ref[t] = (t < F_b and f0_ref[t] > 0), v_deg the same way.
 *   per lag l in [-Lg, Lg]:  O_l = {t : 0 <= t < F_b and 0 <= t + l < F_b};  P_l = {t in O_l : v_ref[t] and
 *     v_deg[t + l]}, n_l = |P_l|;  with x = f0_ref[t], y = f0_deg[t + l] over P_l:  xm = sum x / n, ym = sum y / n,
 *     then in a second pass s_xx = sum (x - xm)^2, s_yy = sum (y - ym)^2, s_xy = sum (x - xm)(y - ym).  The lag is
 *     valid when n_l >= m, s_xx > 0 and s_yy > 0, and then rho_l = s_xy / sqrt(s_xx s_yy) -- exactly 1 for pairwise
 *     identical x and y.
 *   l* is chosen on the walk 0, -1, +1, -2, +2, ..., -Lg, +Lg: the first valid lag whose rho is strictly above every
 *     earlier valid one (an exact tie goes to the smaller |l|, then to the negative lag).
 *   at l*, over P_l*:  e = 12 log2(y / x);  shift_st = sum e / n;  dev_st = sqrt(sum (e - shift_st)^2 / n);
 *     common = n_l*;  voicing = #{t in O_l* : v_ref[t] = v_deg[t + l*]} / |O_l*|.
 *   no valid lag:  rho = 0, lag = 0, common = 0, shift_st = dev_st = 0;  voicing is taken at l = 0, and is 0 when
 *     F_b = 0.
 *   rho, shift_st, dev_st, voicing [B] fp32, each rounded once; lag, common [B] int32.  All but rho may be NULL.
 *   rho is a maximum over lags: an inverted contour reads -1 only at Lg = 0.
 *   One workgroup per row; no atomics, every sum in a fixed order: the same bits on every run.
 *   sa_f0cmp_dim(which): 0 the hop 160 the tracks are taken at, 1 the lag limit 32, 2 threads per workgroup; else
 *     -EINVAL.
 *   -EINVAL, before any launch: a NULL pointer (all outputs but rho may be NULL), B < 1 or > 65535, T < 1 or
 *     > 104858 (the frames of 2^24 samples), max_lag outside 0..32, min_common < 2. */
int sa_f0cmp_dim(int which);
int sa_f0_compare(const float* f0_ref, const float* f0_deg, const int* frames, int B, int T, int max_lag,
                  int min_common, float* rho, int* lag, int* common, float* shift_st, float* dev_st, float* voicing,
                  void* stream);

/* ---- mel-cepstral distortion scoring (sa_mcd.hip; ops.mcd): how far the spectral envelope of one
 * utterance lies from another's, in dB, along a banded dynamic-time-warping alignment.  mel_ref [B][T_ref][n_mels],
 * mel_deg [B][T_deg][n_mels] fp32, log-Mel power in dB (features.Fbank(...)(wav).clamped()); n_ref, n_deg [B] int32,
 * clamped where they are read to N in [0, T_ref] and M in [0, T_deg]; order K: the cepstral coefficients 1..K,
 * 1 <= K <= 32, K < n_mels; band R in 0..63.  A frame at or beyond its row's count is never read into a result.
 * Everything in fp64 on the fp32 inputs:
 *   cepstra   c_k(t) = (1 / n_mels) sum_m mel[t][m] cos(pi k (m + 1/2) / n_mels), k = 1..K.  c_0 is left out: a gain
 *             change costs nothing.
 *   distance  d(i, j) = sqrt(1/2 sum_k (c_k^ref(i) - c_k^deg(j))^2) -- (10 / ln 10) sqrt(2 sum dc^2) written for
 *             cepstra of a dB power spectrum; in dB.
 *   alignment Sakoe-Chiba band, symmetric step weights; only the cells with |i - j| <= R exist:
 *             g(0, 0) = 2 d(0, 0);  g(i, j) = min(g(i-1, j-1) + 2 d(i, j), g(i-1, j) + d(i, j), g(i, j-1) + d(i, j)).
 *   mcd       = g(N-1, M-1) / (N + M): the normaliser does not depend on the path, so the figure is a continuous
 *             function of the inputs, ties between steps change nothing, and no path is traced back.
 *   mcd_sync  = (1 / min(N, M)) sum_{i < min(N, M)} d(i, i): the figure without an alignment.
 *   A row is scored iff N >= 1, M >= 1 and |N - M| <= R: frames = N + M.  Any other row gets mcd = mcd_sync = 0 and
 *   frames = 0.  mcd, mcd_sync [B] fp32, each rounded once; frames [B] int32.
 *   ws: the caller's, 8 B (K (T_ref + T_deg) + (R + 1) (T_ref + T_deg - 1)) bytes, 8-byte aligned (the cepstra of
 *     both inputs and the distances of the band, by anti-diagonal); its contents mean nothing between calls.
 *   Three launches on the given stream (cepstra, band, recurrence: one wave per row over the N + M - 1
 *     anti-diagonals), one path for every T; no copy to the host, no synchronisation, no atomics, every sum in a fixed
 *     order: the same bits on every run.
 *   sa_mcd_dim(which): 0 the band limit 63, 1 the order limit 32, 2 the n_mels limit 128, 3 the T limit 104858 (the
 *     frames of 2^24 samples); else -EINVAL.
 *   -EINVAL, before any launch: a NULL pointer, B < 1 or > 65535 (grid.y), T_ref or T_deg < 1 or > 104858, n_mels < 2
 *     or > 128, order outside 1..32 or >= n_mels, band outside 0..63. */
int sa_mcd_dim(int which);
int sa_mcd(const float* mel_ref, const float* mel_deg, const int* n_ref, const int* n_deg, int B, int T_ref, int T_deg,
           int n_mels, int order, int band, void* ws, float* mcd, float* mcd_sync, int* frames, void* stream);

/* ---- TD-PSOLA pitch modification (sa_psola.hip; ops.psola_marks, ops.psola_plan, ops.psola): the
 * waveform is cut into two-period grains centred on pitch marks, and the same grains are laid down again at the new
 * spacing.  The grains are moved, not altered: the spectral envelope stays, the duration stays, and there is no STFT,
 * no phase, no iteration and no random number.  Every decision is made on integers, or on fp64 formed from the fp32
 * inputs; only the overlap-add rounds.
 *   Per row b:  wav [N] fp32;  f0 [T] fp32 in Hz, <= 0 (or NaN) meaning unvoiced, from either tracker;  rho_q [T]
 *   int32, the ratio per frame in units of 2^-16, clamped to [2^15, 2^17] where it is read (sa_pitch_contour's);
 *   n_valid int32, clamped to [0, N].  T is the frames of the waveform or of the waveform padded to a multiple of
 *   the hop: T = N / 160 + 1 or T = ceil(N / 160) + 1, nothing else.
 *     F_b = min(T, n_valid / 160 + 1);   frame(n) = min((n + 80) / 160, T - 1);   U = 80;
 *     per[t] = (int)clamp(rint(16000.0 / (double)f0[t]), 40, 266) when t < F_b and f0[t] > 0, otherwise 0 (unvoiced).
 *   sa_psola_marks: the analysis marks m_0 < m_1 < ... -> marks [B][Mcap] int32, count [B] int32, Mcap = N / 30 + 2.
 *     The first mark is the argmax of wav over [0, per[0] - 1] if per[0] > 0, otherwise 0.  The mark after m, with
 *     p = per[frame(m)]: the argmax of wav over [m + p - (p >> 2), m + p + (p >> 2)] if p > 0, otherwise m + U (a
 *     window of that one sample).  A mark exists only if its whole window lies below n_valid; the first window that
 *     does not ends the row.  The argmax compares the signed samples with >, a NaN counting as -inf: ties go to the
 *     smallest index and a NaN never wins.  The spacing of the marks is therefore in [30, 332].
 *   sa_psola_plan: where the grains go, in int64 units of 2^-16 samples.  s_0 = m_0 << 16.  For s_j: a(j) is the mark
 *     nearest to s_j -- a pointer that starts at 0 and advances while the next mark is strictly nearer;
 *     P = m_{a+1} - m_a, or m_a - m_{a-1} at the last mark;  r = rho_q[frame(m_a)] if per[frame(m_a)] > 0, otherwise
 *     2^16;  inv = (2^32 + r / 2) / r;  s_{j+1} = s_j + P inv;  while s_j <= m_last << 16.
 *     -> syn_pos[j] = (s_j + 2^15) >> 16 and syn_src[j] = a(j), [B][Jcap] int32, Jcap = N / 15 + 2; syn_count [B].
 *     A row with fewer than 2 marks has no plan: syn_count 0.  ws: the caller's, sa_psola_workspace_bytes(B, N) bytes,
 *     8-byte aligned (P inv per mark); its contents mean nothing between calls.
 *   sa_psola_ola: for n < n_valid, out[n] = (sum_j w wav[m_a + d]) / max(sum_j w, 0.5) over the grains j in ascending
 *     order with d = n - syn_pos[j] inside grain j's support, a = syn_src[j].  Half-widths: L = m_a - m_{a-1} and
 *     R = m_{a+1} - m_a; at the first mark L = R, at the last R = L.  w = 0.5 (1 + cos(pi d / L)) for -L < d < 0, the
 *     same with R for 0 < d < R, 1 at d = 0, formed in fp64 and rounded once to fp32; the products and both sums are
 *     fp32, each rounded on its own (no fused multiply-add), and so is the quotient.  The left side of grain 0 is
 *     rectangular (w = 1) down to source sample 0, the right side of the last grain up to source sample n_valid - 1.
 *     A source index outside [0, n_valid) contributes nothing; a sample no grain reaches is 0.  A row without a plan
 *     is copied, out[n] = wav[n]; out[n] = 0 for n >= n_valid.  Neighbouring halves sum to 1, so at rho_q = 2^16
 *     throughout the plan is the marks themselves and the output is the input.
 *   What the kernels read from device tables is clamped before it is used: n_valid to [0, N], the counts to [0, Mcap]
 *   and [0, Jcap], a mark and a syn_pos to [0, N - 1], syn_src to [0, count - 1], a spacing to [30, 332], rho_q to
 *   [2^15, 2^17] -- none of which changes a table the kernels wrote.  Entries past a row's count mean nothing.
 *   One wave per row (marks, plan), one workgroup per 256 samples (ola); no atomics, every sum in a fixed order, a
 *   row's result does not depend on its neighbours: the same bits on every run and in every batch.
 *   sa_psola_dim(which): 0 U = 80, 1 and 2 the period bounds 40 and 266, 3 and 4 the spacing bounds 30 and 332,
 *     5 samples per workgroup of sa_psola_ola, 6 and 7 the divisors 30 and 15 of Mcap and Jcap; else -EINVAL.
 *   sa_psola_workspace_bytes(B, N): 8 B Mcap, or -EINVAL for a B or N the kernels refuse.
 *   -EINVAL, before any launch: a NULL pointer, B < 1 or > 65535, N < 1 or > 2^24, a T that is neither of the two
 *     above (sa_psola_marks, sa_psola_plan). */
int sa_psola_dim(int which);
long long sa_psola_workspace_bytes(int B, int N);
int sa_psola_marks(const float* wav, const float* f0, const int* n_valid, int B, int N, int T, int* marks, int* count,
                   void* stream);
int sa_psola_plan(const int* marks, const int* count, const float* f0, const int* rho_q, const int* n_valid, int B,
                  int N, int T, void* ws, int* syn_pos, int* syn_src, int* syn_count, void* stream);
int sa_psola_ola(const float* wav, const int* marks, const int* count, const int* syn_pos, const int* syn_src,
                 const int* syn_count, const int* n_valid, int B, int N, float* out, void* stream);

/* ---- LPC formant tracking and its comparison (sa_formants.hip; ops.formant_tracks, ops.formant_compare; DESIGN section
 * 25): where the vocal-tract resonances of a waveform lie, frame by frame, and by which factor each of them moved from
 * one waveform to another.  Sample rate 16000, hop 160, W = 400, order P = 18.
 *   sa_formant_tracks: wav [B][N] fp32; n_valid [B] int32, clamped where it is read to [0, N]; a sample outside
 *   [0, n_valid_b) reads as 0.  T = N / 160 + 1 frames, the frame grid of sa_yin_f0; frame t covers
 *   [160 t - 200, 160 t + 200).  Per frame, everything in fp64 on the fp32 samples:
 *     e[n] = x[n] - 0.97 x[n - 1], e = 0 outside [0, n_valid_b);  f[j] = w[j] e[160 t - 200 + j] with
 *       w[j] = 0.54 - 0.46 cos(2 pi j / 399), j = 0..399.
 *     r_k = sum_j f[j] f[j + k], k = 0..18.  r_0 < 1e-10: the frame is silent (status 1); otherwise r_0 *= 1 + 1e-9.
 *     Levinson-Durbin gives a[0..18]; some |k_i| >= 1 or a prediction error <= 0: a fallback (status 2).
 *     The 18 roots z of a by Aberth-Ehrlich from 0.9 exp(2 pi i (j + 0.25) / 18), until the largest correction is
 *       under 1e-14, at most 64 iterations; no convergence: a fallback (status 2).
 *     A root with Im z > 1e-6 |z| is a candidate: f = arg z 16000 / (2 pi), b = -ln|z| 16000 / pi; it is kept when
 *       90 <= f <= 5500 and b <= 700.
 *     Fewer than three kept: short (status 3).  Otherwise status 0, and F1..F3 and their bandwidths are those of the
 *       three kept candidates of lowest f, in ascending f.
 *   -> freq [B][T][3] and bw [B][T][3] fp32 in Hz, each rounded once, 0 for any status other than 0; status [B][T]
 *   int32.  bw and status may be NULL.  One wave per frame, grid (T, B); one launch on the given stream.
 *   sa_formant_compare: F_ref, F_deg [B][T][3] fp32 and st_ref, st_deg [B][T] int32 (two outputs of
 *   sa_formant_tracks); f0_ref, f0_deg [B][T] fp32 in Hz, 0 or less meaning unvoiced (two tracks of sa_yin_f0 or
 *   sa_f0_viterbi); frames [B] int32, clamped where it is read to F_b in [0, T]; min_common m >= 1.
 *     Frame t counts when t < F_b, st_ref[t] = st_deg[t] = 0, f0_ref[t] > 0 and f0_deg[t] > 0; n of them do.
 *     n >= m:  med_k = the lower median of F_deg[t][k] over the counted frames, the element at index (n - 1) / 2 of the
 *       sorted values (an element of the track: exact);  ratio_k = the lower median of
 *       q_k[t] = fp32((double)F_deg[t][k] / (double)F_ref[t][k]);
 *       shift = fp32(exp((ln ratio_1 + ln ratio_2 + ln ratio_3) / 3)) in fp64 (exactly 1 for ratios of 1);
 *       common = n.
 *     n < m:  med, ratio, shift and common are all 0: the row is not scored.
 *   -> med [B][3], ratio [B][3], shift [B] fp32; common [B] int32.  All but shift may be NULL.
 *   The medians are selected exactly, bit by bit from the top of an order-preserving key of the fp32 values: 33 passes
 *   over the row by one workgroup, one path for every T, no workspace.  The same order holds for values of any sign;
 *   a NaN sorts past the infinity of its sign.
 *   No copy to the host, no synchronisation, no atomics, every sum in a fixed order: the same bits on every run.
 *   sa_formant_dim(which): 0 W = 400, 1 the hop 160, 2 P = 18, 3 the 3 formants, 4 threads per workgroup of
 *     sa_formant_tracks, 5 the iteration limit 64, 6 the T limit 104858 of sa_formant_compare (the frames of 2^24
 *     samples), 7 threads per workgroup of sa_formant_compare; else -EINVAL.
 *   -EINVAL, before any launch: a NULL required pointer, B < 1 or > 65535, N < 1 or > 2^24 (sa_formant_tracks),
 *     T < 1 or > 104858 and min_common < 1 (sa_formant_compare). */
int sa_formant_dim(int which);
int sa_formant_tracks(const float* wav, const int* n_valid, int B, int N, float* freq, float* bw, int* status,
                      void* stream);
int sa_formant_compare(const float* F_ref, const float* F_deg, const int* st_ref, const int* st_deg,
                       const float* f0_ref, const float* f0_deg, const int* frames, int B, int T, int min_common,
                       float* med, float* ratio, float* shift, int* common, void* stream);

/* ---- LPC formant normalisation (sa_formant_norm.hip; formantnorm.py, ops.pole_warp, ops.formant_centre; DESIGN
 * section 26): every complex LPC pole's angle scaled by a ratio q per utterance, and the q that brings an utterance's
 * own tracked formants to a target.  Sample rate 16000.
 *   sa_pole_warp: wav [B][N] fp32, q [B] fp32, n_valid [B] int32 -> out [B][N] fp32, out != wav.  Everything is
 *   sa_mcadams's (above), word for word: frames of W = 320 at hop H = 160 under the periodic sqrt-Hann window w,
 *   T = (N + 159) / 160 + 1 of them, frame t over [160 t - 160, 160 t + 160); a sample outside [0, n_valid_b) reads
 *   as 0.  Per frame, in fp64:
 *     f = w x;  r_k = sum_j f[j] f[j + k], k = 0..20;  r_0 < 1e-10: silent (status 1), rec = f;  r_0 *= 1 + 1e-9;
 *     a[0..20] by Levinson-Durbin; some |k_i| >= 1 or a prediction error <= 0: fallback (status 2), rec = f;
 *     the 20 roots z of a by Aberth-Ehrlich from 0.9 exp(2 pi i (j + 0.25) / 20), stopped when the largest
 *       correction is under 1e-14, given up (fallback) after 64 iterations;  a root is real when
 *       |Im z| <= 1e-6 |z|, kept when Im z > 1e-6 |z|, dropped otherwise;  2 kept + real != 20: fallback;
 *     a' = prod_real (1 - Re z x) prod_kept (1 - 2 |z| cos(phi') x + |z|^2 x^2), phi = arg z and
 *       phi' = q phi                                               for phi <= phi0,
 *       phi' = q phi0 + (pi - q phi0) (phi - phi0) / (pi - phi0)   above it,   phi0 = 0.85 pi min(1, 1 / q):
 *       continuous, strictly increasing, (0, pi) onto itself; |z| and the real poles are kept;
 *     res = FIR(a) f, rec = IIR(1 / a') res, both from zero history;  the frame stored is fp32(rec w).
 *   y[n] = F_t0[n - 160 t0 + 160] + F_{t0 + 1}[n - 160 t0], t0 = n / 160 (fp32);  out[n] = fp32(g_b y[n]) for
 *   n < n_valid_b and 0 from there on;  level != 0: g_b = sqrt(sum x^2 / sum y^2) over n < n_valid_b (fp64, a fixed
 *   order; 1 when either sum is 0), else 1.  q is read on the device: a value outside [0.5, 2] is taken as the nearer
 *   bound, a NaN as 1; a row whose q is 1 is copied bit for bit below n_valid_b (gain 1, status 0).  n_valid_b is
 *   clamped to [0, N].  The same bits on every run.
 *   ws: the caller's, 4 B T 320 + 8 (2 B ceil(N / C) + B) bytes, 8-byte aligned, C = sa_pole_warp_dim(6); its
 *     contents mean nothing between calls.  status: NULL, or int32 [B][T].  gain: NULL, or fp32 [B].
 *   sa_pole_warp_dim(which): 0 W 320, 1 H 160, 2 P 20, 3 frames per workgroup, 4 threads per workgroup, 5 the largest
 *     iteration count 64, 6 samples per block of the level sums, 7 the knee 0.85 in thousandths (850); else -EINVAL.
 *   -EINVAL, before any launch: a NULL pointer (status and gain may be NULL), B < 1 or > 65535 (grid.y), N < 1 or
 *     > 2^30, T > 2^23.
 *   sa_formant_centre: freq [B][T][3] fp32 and status [B][T] int32 (one output of sa_formant_tracks); f0 [B][T] fp32 in
 *   Hz, 0 or less meaning unvoiced, or NULL: every frame voiced; frames [B] int32, clamped where it is read to F_b in
 *   [0, T]; the target t1 < t2 < t3 in Hz; q_min <= 1 <= q_max; min_frames m >= 1.
 *     Frame t counts when t < F_b, status[t] = 0 and f0[t] > 0; n of them do.
 *     n >= m:  med_k = the lower median of freq[t][k] over the counted frames, the element at index (n - 1) / 2 of the
 *       sorted values (an element of the track: exact);
 *       q = fp32(clamp(exp((ln(t1 / med_1) + ln(t2 / med_2) + ln(t3 / med_3)) / 3), q_min, q_max)) in fp64 (exactly 1
 *       when the medians are the target; 1 when the value is a NaN, which takes a median of 0 or less);  count = n.
 *     n < m:  med = 0, q = 1, count = 0: the row is left as it is.
 *   -> med [B][3] fp32, q [B] fp32, count [B] int32.  med and count may be NULL.  One workgroup of 16 waves per row, the
 *   medians by sa_formant_compare's bitwise select on three keys; no workspace, no atomics, the same bits on every run.
 *   -EINVAL, before any launch: a NULL required pointer, B < 1 or > 65535, T < 1 or > 104858, a target that is not
 *     90 <= t1 < t2 < t3 <= 5500, bounds that are not 0.5 <= q_min <= 1 <= q_max <= 2, min_frames < 1. */
int sa_pole_warp_dim(int which);
int sa_pole_warp(const float* wav, const float* q, const int* n_valid, int B, int N, int level, float* out, void* ws,
                 int* status, float* gain, void* stream);
int sa_formant_centre(const float* freq, const int* status, const float* f0, const int* frames, int B, int T, float t1,
                      float t2, float t3, float q_min, float q_max, int min_frames, float* med, float* q, int* count,
                      void* stream);

/* ---- LPC source-filter resynthesis (sa_srcfilt.hip; sourcefilter.py, ops.srcfilt_pulses, ops.srcfilt_excite,
 * ops.srcfilt_synth, ops.srcfilt): the classic LPC vocoder.  Every frame keeps its all-pole envelope
 * and its energy; its residual is discarded and the filter is driven by a synthetic excitation, pulses at the F0 track
 * where the frame is voiced and noise elsewhere.  The pulses are laid down at the period asked for, so the same pass
 * sets the pitch.  No STFT, no phase, no pitch marks, no iteration, no root finder, no copy to the host.  Every decision
 * of the first two entry points is made on integers, or on fp64 formed from the fp32 inputs; only the filtered output
 * rounds.  Sample rate 16000; W = 320, H = 160, P = 20 and the periodic sqrt-Hann window w are sa_mcadams's.
 *   Per row b: n_valid int32, clamped to [0, N]; a sample outside [0, n_valid_b) reads as 0 and is written as 0.
 *   f0 [T] fp32 in Hz from either tracker, T = N / 160 + 1 or T = ceil(N / 160) + 1 (what sa_psola_marks accepts),
 *   nothing else.  frame(n) = min((n + 80) / 160, T - 1).  Frame t is voiced when f0[t] > 0 and f0[t] < +inf: a NaN,
 *   a negative value and an infinity are unvoiced.  Positions are int64 in units of 2^-16 samples.
 *   sa_srcfilt_pulses: f0 [B][T] fp32; rho_q [B][T] int32, the pitch ratio per frame in units of 2^-16, or NULL;
 *   n_valid [B] int32 -> pos_q [B][Kcap] int64, period_q [B][Kcap] int32, count [B] int32, Kcap = N / 40 + 2.
 *     rho = clamp(rho_q[t], 2^15, 2^17), 2^16 when rho_q is NULL.
 *     P_q[t] = (int)clamp(rint(16000 2^32 / ((double)f0[t] (double)rho)), 40 2^16, 266 2^16): the denominator is exact
 *       in fp64 (24 by 18 bits), the quotient is rounded once, rint rounds half to even, and the clamp is applied in
 *       fp64 before the conversion.  A ratio above 1 raises the pitch, so rho divides the period.
 *     The walk starts at s = 0 and runs while floor(s / 2^16) < n_valid_b, with t = frame(floor(s / 2^16)):
 *       voiced: emit (pos_q, period_q) = (s, P_q[t]), then s += P_q[t];
 *       unvoiced and t = T - 1: stop;   unvoiced otherwise: s = (160 t + 80) 2^16, the first sample of frame t + 1.
 *     Pulses are 40 samples or more apart and a row has at most N / 40 + 1 of them.  Every step moves s forward, so
 *     the walk ends; the kernel also stops after Kcap + T steps.  Entries past a row's count mean nothing.
 *   sa_srcfilt_excite: f0, the table of sa_srcfilt_pulses, seed [B] int32, n_valid [B], aspiration -> exc [B][N] fp32.
 *     mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16, in uint32.
 *     k_b = mix((uint32)seed_b);  h = mix((uint32)n ^ k_b);  u_n = ((int)(h >> 8) - 2^23) 2^-23: exact in fp32, in
 *     [-1, 1).  For n < n_valid_b, every fp32 operation rounded on its own and none contracted:
 *       e = c u_n, c = aspiration when frame(n) is voiced and 1 otherwise;
 *       the pulse k with floor(s_k / 2^16) = n adds A_k (1 - phi_k);
 *       the pulse k with floor(s_k / 2^16) + 1 = n and phi_k > 0 adds A_k phi_k;
 *       phi_k = (s_k mod 2^16) 2^-16;  A_k = fp32(sqrt((double)P_k 2^-16)), which gives the pulse train unit mean power.
 *     exc[n] = e, and 0 for n >= n_valid_b.  A sample receives at most one pulse term (the spacing is 40 or more), so
 *     there is no order to fix.  Uniform noise has power 1 / 3: a voiced frame's noise lies at aspiration^2 / 3 of the
 *     pulses' power.  period_q is clamped to [40 2^16, 266 2^16] and count to [0, Kcap] where they are read; pos_q is
 *     only compared.  (Left open by the feature's statement and settled here: the entry point takes f0 and T, since
 *     the noise level of a sample depends on its frame's voicing; the last pulse's second term falls away when its
 *     sample is n_valid_b.)
 *   sa_srcfilt_synth: wav [B][N] fp32 (the envelope and the level), exc [B][N] fp32, n_valid [B] -> out [B][N] fp32,
 *   out != wav, out != exc.  sa_mcadams's framing: T' = (N + 159) / 160 + 1 frames, frame t over
 *   [160 t - 160, 160 t + 160).  Per frame, in fp64, f = w x and ex = w e:
 *     (a) r_k = sum_j f[j] f[j + k], k = 0..20;  r_0 < 1e-10: silent (status 1), rec = f;
 *     (b) r_0 *= 1 + 1e-9;  a[0..20] by Levinson-Durbin with the final prediction error E = r_0 prod (1 - k_i^2), formed
 *         step by step;  some |k_i| >= 1 or an error <= 0: fallback (status 2), rec = f;
 *     (c) Ee = sum_j ex[j]^2;  Ee < 1e-20: no excitation (status 3), rec = 0;  otherwise g = sqrt(E / Ee);
 *     (d) rec = IIR(1 / a)(g ex) from zero history: rec[j] = g ex[j] - sum_{k=1..20} a[k] rec[j - k];
 *     (e) the frame stored is fp32(rec w).
 *   y[n] = F_t0[n - 160 t0 + 160] + F_{t0 + 1}[n - 160 t0], t0 = n / 160 (fp32);  out[n] = fp32(g_b y[n]) for
 *   n < n_valid_b and 0 from there on;  level != 0: g_b = sqrt(sum x^2 / sum y^2) over n < n_valid_b (fp64, a fixed
 *   order; 1 when either sum is 0), else 1.  No setting is an identity, so no row is ever copied.
 *   ws: the caller's, sa_srcfilt_workspace_bytes(B, N) = 4 B T' 320 + 8 (2 B ceil(N / C) + B) bytes (sa_mcadams's
 *     layout), 8-byte aligned, C = sa_srcfilt_dim(4); its contents mean nothing between calls.  status: NULL, or int32
 *     [B][T'].  gain: NULL, or fp32 [B].
 *   One wave per row (pulses), one workgroup per 256 samples (excite), one wave per frame (synth); no atomics, every
 *   sum in a fixed order, a row's result does not depend on its neighbours: the same bits on every run and in every
 *   batch.
 *   sa_srcfilt_dim(which): 0 W 320, 1 H 160, 2 P 20, 3 threads per frame, 4 samples per block of the level sums, 5 and
 *     6 the period bounds 40 and 266, 7 the divisor 40 of Kcap, 8 samples per workgroup of sa_srcfilt_excite, 9 pulses
 *     staged per workgroup there; else -EINVAL.
 *   sa_srcfilt_workspace_bytes(B, N): the size above, or -EINVAL for a B or N the kernels refuse.
 *   -EINVAL, before any launch: a NULL required pointer (rho_q, status and gain may be NULL), B < 1 or > 65535,
 *     N < 1 or > 2^24, a T that is neither of the two above (pulses, excite), an aspiration outside [0, 1] (a NaN
 *     too). */
int sa_srcfilt_dim(int which);
long long sa_srcfilt_workspace_bytes(int B, int N);
int sa_srcfilt_pulses(const float* f0, const int* rho_q, const int* n_valid, int B, int N, int T, long long* pos_q,
                      int* period_q, int* count, void* stream);
int sa_srcfilt_excite(const float* f0, const long long* pos_q, const int* period_q, const int* count, const int* seed,
                      const int* n_valid, int B, int N, int T, float aspiration, float* exc, void* stream);
int sa_srcfilt_synth(const float* wav, const float* exc, const int* n_valid, int B, int N, int level, float* out,
                     void* ws, int* status, float* gain, void* stream);

/* ---- modulation-spectrum smoothing (sa_modspec.hip; modspec.py, ops.modspec_smooth): every STFT
 * bin's log-magnitude trajectory is low-pass filtered along time by a symmetric FIR, the input's phases are kept, and
 * the caller inverts once.  The only transform here that acts between frames.  n_fft 400, hop 160, 201 bins, 100
 * frames a second.
 *   R, C: [B][T][201] complex64 (interleaved re, im fp32), C != R.
 *   taps: device fp64 [J + 1], the half h[0..J] of a symmetric FIR along time, used as given (ops.modspec_taps
 *     normalises it to h0 + 2 sum h_j = 1).
 *   depth: [B] fp32, read on the device; a value outside [0, 1] is taken as the nearer bound and a NaN as 0.
 *   frames: [B] int32, clamped to [0, T]: T_b, the frames of row b that count.
 *   peak: [B] fp64, receives peak_b (0 for a row with T_b = 0).
 *   Lout: NULL, or fp64 [B][T][201], receives L + g (tests); 0 for t >= T_b.
 *   Per row b, in fp64 formed from the fp32 values:
 *     m[t][k] = sqrt(re^2 + im^2): the products are exact, the sum and the root are rounded once each;
 *     peak_b = max over t < T_b and all k of m (a maximum is exact in any order);
 *     fl_b = max(floor_rel peak_b, 1e-10);   L[t][k] = ln(max(m, fl_b));
 *     for t < T_b:  s = h0 L[t] + sum_{j = 1..J} h_j (L[c(t - j)] + L[c(t + j)]), j ascending, c(i) = clamp(i, 0,
 *       T_b - 1) (edge replication, as sa_pitch_contour does); each pair is added first, and its product with h_j is
 *       fused into the running sum (one rounding per j after the pair's);
 *     g = clamp(d_b (s - L[t]), +-max_gain_ln);
 *     C[t][k] = (fp32(re e^g), fp32(im e^g)), each rounded once from the fp64 product.
 *   The phase is kept by construction: no atan2, no division; R = 0 gives C = 0.
 *   Copied bit for bit from R: the frames t >= T_b of every row, and every frame of a row with d_b = 0 (after the
 *   clamp) or T_b = 0.  J = 0 with h0 = 1 gives C = R by arithmetic (g = 0).
 *   R is taken as finite; what a non-finite value spoils is unspecified.  No address depends on data.
 *   Two launches: the row peak as per-workgroup partial maxima of re^2 + im^2 into ws (the root is monotonic, so the
 *   root of the largest sum is the largest root), reduced by every workgroup of the second launch that reads them;
 *   then the smoothing pass, one workgroup per (sa_modspec_dim(4) frames) x (sa_modspec_dim(5) bins) tile, which
 *   stages fp64 L of the tile and J frames either side in LDS.  No atomics, every sum in a fixed order, no workgroup
 *   waits on another, a row's result does not depend on its neighbours: the same bits on every run and in every batch.
 *   ws: the caller's, sa_modspec_workspace_bytes(B, T) = 8 B min(ceil(T / 64), 256) bytes, 8-byte aligned; its
 *     contents mean nothing between calls.
 *   sa_modspec_dim(which): 0 n_fft 400, 1 hop 160, 2 bins 201, 3 the largest J 64, 4 frames per workgroup 128,
 *     5 bins per workgroup 16, 6 consecutive frames per thread 8, 7 the most partial maxima per row 256, 8 the fewest
 *     frames per partial maximum 64; else -EINVAL.
 *   sa_modspec_workspace_bytes(B, T): the size above, or -EINVAL for a B or T the kernels refuse.
 *   -EINVAL, before any launch: a NULL pointer (Lout may be NULL), C == R, B < 1 or > 65535, T < 1 or > 2^23, J outside
 *     0..64, floor_rel outside (0, 1) (a NaN too), max_gain_ln <= 0 (a NaN too). */
long long sa_modspec_workspace_bytes(int B, int T);
int sa_modspec_dim(int which);
int sa_modspec_smooth(const void* R, const double* taps, int J, const float* depth, const int* frames, int B, int T,
                      float floor_rel, float max_gain_ln, void* C, double* peak, double* Lout, void* ws, void* stream);

/* ---- WSOLA time-scale modification (sa_wsola.hip; ops.wsola_quant, ops.wsola_search, ops.wsola_ola, ops.wsola;
 * timescale.py): windows of W = 320 samples of the input are copied to the output at a hop of
 * H = 160, and each window's position is chosen within D = 160 samples of where the tempo says it should be, so that it
 * continues the previous one.  The samples are moved, not altered: pitch and envelope stay, the duration changes, and
 * there is no STFT, no phase, no iteration and no random number.  Every decision is made on integers; the overlap-add
 * is two fp32 products and one fp32 sum.  tests/wsola_ref.py restates all of it and agrees with the kernels exactly.
 *   Per row b:  wav [N] fp32;  n_valid int32, clamped to [0, N];  tempo_q int32 in units of 2^-16, clamped to
 *   [2^15, 2^17] where it is read; above 2^16 is faster, a shorter output.
 *   1. Length.  n_out = min(Nout, (n_valid 2^16 + tempo_q / 2) / tempo_q) in int64 (/ truncates), 0 when n_valid = 0;
 *     K = (n_out - 1) / H + 1, 0 when n_out = 0.  sa_wsola_out_len(n, tempo_q) is the same figure before the cap.
 *   2. Search signal.  s = the largest finite |wav[n]|, n < n_valid.  q[n] = rint((double)wav[n] 16383 / (double)s) as
 *     int16: the product is exact, the division rounds once, ties go to even.  q[n] = 0 where the sample is not
 *     finite, where s = 0, and for n >= n_valid; a q read outside [0, n_valid) is 0.
 *   3. Positions.  p_0 = 0.  For k = 1 .. K - 1, with int64 products: a = (k H tempo_q + 2^15) >> 16 and
 *     t = p_{k-1} + H.  The candidates c are the integers of [lo, hi], lo = max(a - D, 0), hi = min(a + D,
 *     max(n_valid - 1, 0)); when hi < lo the one candidate is hi.  cost(c) = sum_{n < W} |q[t + n] - q[c + n]|, an
 *     integer below 2^24 and so exact in any order.  p_k is the candidate of least cost; ties go to the smallest
 *     |c - a|, then to the smaller c.  A silent or constant stretch therefore follows a; at tempo_q = 2^16 the cost at
 *     c = t = a is 0 and p_k = k H.
 *   4. Overlap-add.  For m < n_out, k = m / H, r = m - k H;  X(i) = wav[i] for 0 <= i < n_valid and 0 elsewhere;
 *     hann[j] = 0.5 - 0.5 cos(2 pi j / W), j < W, formed in fp64 by the caller and rounded once (a table of W floats:
 *     a device cosine may round differently).  out[m] = X(p_k + r), the sample's own bits, when k = 0 or
 *     p_k = p_{k-1} + H (both windows hold the same sample there: contiguous stretches and the whole of tempo 1 are
 *     copies).  Otherwise out[m] = fl(fl(hann[r] X(p_k + r)) + fl(hann[r + H] X(p_{k-1} + H + r))) in fp32, each
 *     operation rounded on its own, no fused multiply-add; a sum that is a NaN is written as 0x7fc00000 (which NaN
 *     an invalid operation gives is not the same on every machine).  out[m] = 0 for n_out <= m < Nout.
 *   Outputs: out [B][Nout] fp32;  pos [B][Kcap] int32, Kcap = (Nout - 1) / H + 1, entries from count on mean nothing;
 *   count [B] = K;  n_out [B].
 *   sa_wsola_quant: two launches, the partial maxima of every 4096 samples and then q, int16 [B][N] at the start of
 *     ws; the rest of ws holds the partial maxima.  ws: the caller's, sa_wsola_workspace_bytes(B, N) bytes, 16-byte
 *     aligned.  sa_wsola_search: one workgroup per row walks step 3 over q staged through LDS sa_wsola_dim(4) samples
 *     at a time, and writes pos, count and n_out.  sa_wsola_ola: step 4; it forms n_out from n_valid and tempo_q as
 *     step 1 does, reads count (clamped to [0, Kcap]; a sample of a frame from count on is 0) and pos (clamped to
 *     [0, N]) -- none of which changes tables sa_wsola_search wrote.  sa_wsola: the three in a row.
 *   No atomics, fixed orders, a row's result does not depend on its neighbours: the same bits on every run and in
 *   every batch.
 *   sa_wsola_dim(which): 0 H = 160, 1 W = 320, 2 D = 160, 3 Q = 16383, 4 the samples per staged chunk of the search,
 *     5 the samples per workgroup of the overlap-add, 6 the samples per partial maximum; else -EINVAL.
 *   sa_wsola_out_len(n, tempo_q): step 1's quotient, or -EINVAL for n < 0 or > 2^24.
 *   sa_wsola_workspace_bytes(B, N): 2 B N rounded up to 16, plus 4 B ceil((N + 3) / 4096) rounded up to 16; -EINVAL
 *     for a B or N the kernels refuse.
 *   -EINVAL, before any launch: a NULL pointer, B < 1 or > 65535, N < 1 or > 2^24, Nout < 1 or > 2^25, out
 *     overlapping wav (sa_wsola_ola, sa_wsola). */
int sa_wsola_dim(int which);
int sa_wsola_out_len(int n, int tempo_q);
long long sa_wsola_workspace_bytes(int B, int N);
int sa_wsola_quant(const float* wav, const int* n_valid, int B, int N, void* ws, void* stream);
int sa_wsola_search(const void* ws, const int* tempo_q, const int* n_valid, int B, int N, int Nout, int* pos,
                    int* count, int* n_out, void* stream);
int sa_wsola_ola(const float* wav, const int* pos, const int* count, const int* tempo_q, const int* n_valid,
                 const float* hann, int B, int N, int Nout, float* out, void* stream);
int sa_wsola(const float* wav, const int* tempo_q, const int* n_valid, const float* hann, int B, int N, int Nout,
             void* ws, float* out, int* pos, int* count, int* n_out, void* stream);

/* ---- element-wise passes of the frozen recogniser (sa_asr.hip; SURVEY 8f-2, models/SpeechBrain_ASR.py:16-30;
 * bf16 storage, fp32 arithmetic; the GEMMs around them are library calls).
 *   sa_add_layernorm_fwd: s = bf16(x + r) (r may be NULL), y = LayerNorm_d(s) * gamma + beta over rows of d
 *     elements (d in {256, 512, 768, 1024}); s_out (the tensor the backward re-reads) and stat [rows][2] =
 *     (mean, rstd) are optional: NULL under no_grad.  speechbrain's post-norm layers, x = norm(x + f(x)).
 *   sa_layernorm_bwd: d s from d y, s, stat, gamma -- the gradient of both addends of the forward.
 *   sa_reflect_pad_fwd / _bwd: F.pad(., (1, 1, 1, 1), "reflect") on the (T, F) axes of [B][T][F][C] rows
 *     (the "same" padding of ConvolutionFrontEnd's 3 x 3 convolutions) and its adjoint; T, F >= 3. */
int sa_add_layernorm_fwd(const void* x, const void* r, const void* gamma, const void* beta, void* y, void* s_out,
                         float* stat, int rows, int d, float eps, void* stream);
int sa_layernorm_bwd(const void* dy, const void* s, const float* stat, const void* gamma, void* ds, int rows,
                     int d, void* stream);
/* sa_ln_leaky_fwd / _bwd: the front end's LayerNorm over (frequency, channel) + LeakyReLU in one pass each way;
 *   rows of d in {5120, 10240} elements (-ENOSYS otherwise); the backward recomputes the activation's branch
 *   from x and stat, so only x (the convolution's output) and [rows][2] statistics are kept. */
int sa_ln_leaky_fwd(const void* x, const void* gamma, const void* beta, void* y, float* stat, int rows, int d,
                    float eps, float slope, void* stream);
int sa_ln_leaky_bwd(const void* dy, const void* x, const float* stat, const void* gamma, const void* beta, void* dx,
                    int rows, int d, float slope, void* stream);
/* sa_asr_block0_fwd / _bwd: block 0 of the front end -- Conv2d(1 -> C = 128, 3 x 3, stride 2, reflect "same"
 *   padding) + LayerNorm over (F' = 40, C) + LeakyReLU on x [B][T][F = 80] -> y [B][ceil(T/2)][40][128] -- as one
 *   pass each way (-ENOSYS for other F / C).  w [C][3][3], bias [C], gamma / beta [40][128], all bf16.
 *   stat [B * ceil(T/2)][2] (mean, rstd; NULL under no_grad) is all the backward keeps besides x: it recomputes
 *   the convolution.  part: fp32 scratch [B * ceil(T/2)][3][F + 2]; dx [B][T][F] bf16. */
int sa_asr_block0_fwd(const void* x, const void* w, const void* bias, const void* gamma, const void* beta, void* y,
                      float* stat, int B, int T, int F, int C, float eps, float slope, void* stream);
int sa_asr_block0_bwd(const void* dy, const void* x, const void* w, const void* bias, const void* gamma,
                      const void* beta, const float* stat, float* part, void* dx, int B, int T, int F, int C,
                      float slope, void* stream);
int sa_reflect_pad_fwd(const void* x, void* y, int B, int T, int F, int C, void* stream);
int sa_reflect_pad_bwd(const void* dy, void* dx, int B, int T, int F, int C, void* stream);

/* ---- data-parallel exchange (sa_comm.hip): what DistributedDataParallel / SyncBatchNorm do for
 * the reference once speechbrain_convae_train.py:524 (ddp_init_group) has run -- the gradient
 * average and the BatchNorm statistic sums -- as in-place RCCL all-reduces on a side stream the
 * library owns.  One process per GPU; rank 0 calls sa_comm_unique_id and hands the 128 bytes to
 * the other ranks by any host channel (the Python side uses the torch.distributed store), then
 * every rank calls sa_comm_init (collective: returns when all `world` ranks have joined).
 *   sa_comm_allreduce: the side stream waits for everything enqueued so far on `producer_stream`,
 *     then reduces buf[n] in place (dtype SA_F32 | SA_F64; avg != 0: ncclAvg, else sum).  Returns
 *     at once.  sa_comm_allreduce_inline: the same collective enqueued in `stream` itself (no side
 *     stream, no events: producer and consumer are that stream's neighbours).  sa_comm_join: `consumer_stream` waits for every all-reduce enqueued so far.
 *   Codes: -ENOSYS no RCCL library in the process or on the loader path (it is bound by dlopen
 *     at the first sa_comm_* call, never at load time), -ENOTCONN before sa_comm_init, -EEXIST
 *     second sa_comm_init, -(1000 + ncclResult_t) from RCCL, -(hipError_t) from HIP.
 *   sa_comm_world: 0 before init.  sa_comm_ncalls: all-reduces enqueued since init (tests). */
int sa_comm_unique_id(void* id128);
int sa_comm_init(int rank, int world, const void* id128, int device);
int sa_comm_world(void);
int sa_comm_allreduce(void* buf, long long n, int dtype, int avg, void* producer_stream);
int sa_comm_allreduce_inline(void* buf, long long n, int dtype, int avg, void* stream);
int sa_comm_join(void* consumer_stream);
int sa_comm_ncalls(void);
int sa_comm_destroy(void);

#ifdef __cplusplus
}
#endif
#endif /* SA_HIP_H */
