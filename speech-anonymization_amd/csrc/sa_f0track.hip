// Viterbi F0 tracking (pitchnorm.f0_track(method="viterbi")) on the d' rows sa_yin_f0 writes:
//   sa_f0_candidates   per frame the K = 8 dips of d' with the smallest (cost, lag), in ascending lag
//   sa_f0_viterbi      per row the cheapest path through the frames' candidates and an unvoiced state, its
//                      backtrace, and the parabolic refinement of the chosen lags (sa_yin_f0's expression)
// Costs are Q16 integers and every path sum an int64: no floating point decides anything after the candidates'
// costs are rounded.  Plain HIP C++, no atomics, the same bits on every run.
#include "sa_common.h"
#include "sa_pitch_shared.h"
#include <errno.h>
#include <limits.h>
#include <math.h>

#define FV_ROW (PN_TMAX + 1)             // d' values per frame
#define FV_K 8                           // candidates per frame
#define FV_S (FV_K + 1)                  // states: the candidates, then unvoiced
#define FV_G 8                           // frames per workgroup of sa_f0_candidates, one wave each
#define FV_LAGS 5                        // consecutive lags per lane
#define FV_CHUNK 256                     // frames per staged chunk of sa_f0_viterbi
#define FV_FRAC 16
#define FV_ONE (1 << FV_FRAC)
#define FV_INF (1LL << 62)

extern "C" int sa_f0v_dim(int which) {
  switch (which) {
    case 0: return FV_K;
    case 1: return FV_S;
    case 2: return FV_G;
    case 3: return FV_CHUNK;
    case 4: return FV_FRAC;
    default: return -EINVAL;
  }
}

// ---- candidates --------------------------------------------------------------------------------------
// grid (tiles of 8 frames, B), 8 waves; wave f takes frame t0 + f and stages its d' row.  Lane l owns the lags
// 5 l + 1 .. 5 l + 5 and keys its dips with (q << 9) | tau (q <= 2^16, tau < 2^9: the order of (q, tau)).  Eight
// rounds of a butterfly minimum name the winners, smallest first; the lane that held a winner retires it.  Lane
// r < 8 then places winner r at the rank of its lag among the winners; the slots past the last winner get (-1, 0).
__global__ __launch_bounds__(FV_G * SA_WAVE) void sa_f0_candidates_kernel(const float* __restrict__ dprime, int T,
                                                                          int* __restrict__ cand_tau,
                                                                          int* __restrict__ cand_q) {
  __shared__ float dp[FV_G][FV_ROW + 1];
  const int tid = threadIdx.x, b = blockIdx.y, f = tid >> 6, lane = tid & 63, t = blockIdx.x * FV_G + f;
  if (t < T) {
    const float* row = dprime + ((size_t)b * T + t) * FV_ROW;
    for (int i = lane; i < FV_ROW; i += SA_WAVE) dp[f][i] = row[i];
  }
  __syncthreads();
  if (t >= T) return;

  int key[FV_LAGS];
#pragma unroll
  for (int k = 0; k < FV_LAGS; ++k) {
    const int tau = FV_LAGS * lane + 1 + k;
    key[k] = INT_MAX;
    if (tau >= PN_TMIN && tau < PN_TMAX) {
      const float c = dp[f][tau];
      if (c <= dp[f][tau - 1] && c < dp[f][tau + 1]) {
        const int q = (int)rintf(fminf(fmaxf(c, 0.0f), 1.0f) * (float)FV_ONE);
        key[k] = (q << 9) | tau;
      }
    }
  }
  int win[FV_K];
#pragma unroll
  for (int r = 0; r < FV_K; ++r) {
    int m = key[0];
#pragma unroll
    for (int k = 1; k < FV_LAGS; ++k) m = min(m, key[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o, 64));
    win[r] = m;
    if (m != INT_MAX) {
#pragma unroll
      for (int k = 0; k < FV_LAGS; ++k)
        if (key[k] == m) key[k] = INT_MAX;
    }
  }
  if (lane < FV_K) {
    int mine = INT_MAX;
#pragma unroll
    for (int r = 0; r < FV_K; ++r)
      if (r == lane) mine = win[r];
    const size_t o = ((size_t)b * T + t) * FV_K;
    if (mine == INT_MAX) {               // winners come smallest first: round `lane` found none, its slot is unused
      cand_tau[o + lane] = -1;
      cand_q[o + lane] = 0;
    } else {
      const int tau = mine & 511;
      int rank = 0;
#pragma unroll
      for (int r = 0; r < FV_K; ++r)
        if (win[r] != INT_MAX && (win[r] & 511) < tau) ++rank;
      cand_tau[o + rank] = tau;
      cand_q[o + rank] = mine >> 9;
    }
  }
}

extern "C" int sa_f0_candidates(const float* dprime, int B, int T, int* cand_tau, int* cand_q, void* stream) {
  if (!dprime || !cand_tau || !cand_q || !pn_rows_ok(B) || !pn_frames_ok(T, 1)) return -EINVAL;
  hipLaunchKernelGGL(sa_f0_candidates_kernel, dim3(sa_div_up(T, FV_G), B), dim3(FV_G * SA_WAVE), 0,
                     (hipStream_t)stream, dprime, T, cand_tau, cand_q);
  return -(int)hipGetLastError();
}

// ---- decode ------------------------------------------------------------------------------------------
// grid (B), one wave per row.  Forward, in chunks of 256 frames: the wave stages, per frame and candidate, the lag
// (clamped; -1 absent), LOG[lag] and the local cost; then lane s <= 8 owns target state s and walks the nine
// predecessors by lane reads (int64 delta, LOG of the predecessor's lag), taking a predecessor only when it is
// strictly cheaper than the ones before it -- ties go to the smaller index.  psi collects in LDS and leaves for the
// caller's workspace once per chunk.  Backward, chunk by chunk from the end: psi comes back to LDS, the wave follows it
// (every lane the same walk: broadcast reads), and the lanes write path and f0 of the chunk's frames in parallel.
// The frames that count are sa_pitch_ratio's and the refinement of a chosen lag is sa_yin_f0's: one text each,
// sa_pitch_shared.h.

// lane a's value in every lane; a is the same in all lanes (an unrolled loop's counter), so this is a scalar read of
// the register, not a trip through LDS
__device__ static inline int fv_from(int v, int a) { return __builtin_amdgcn_readlane(v, a); }
__device__ static inline long long fv_from(long long v, int a) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffLL), a);
  const int hi = __builtin_amdgcn_readlane((int)(v >> 32), a);
  return ((long long)hi << 32) | (long long)lo;
}

__device__ static inline int fv_lag(int tau) { return tau < 0 ? -1 : min(max(tau, PN_TMIN), PN_TMAX - 1); }

__global__ __launch_bounds__(SA_WAVE) void sa_f0_viterbi_kernel(const float* __restrict__ dprime,
                                                                const int* __restrict__ cand_tau,
                                                                const int* __restrict__ cand_q,
                                                                const float* __restrict__ lens,
                                                                const int* __restrict__ log_q, int T, int N,
                                                                long long vq, unsigned sq, unsigned jq,
                                                                long long bq, unsigned char* __restrict__ psi,
                                                                int* __restrict__ path, float* __restrict__ f0) {
  __shared__ int lgt[FV_ROW];
  __shared__ int c_tau[FV_CHUNK * FV_K], c_lg[FV_CHUNK * FV_K];
  __shared__ long long c_loc[FV_CHUNK * FV_K];
  __shared__ unsigned char c_psi[FV_CHUNK * FV_S];
  __shared__ int c_path[FV_CHUNK];
  const int lane = threadIdx.x, b = blockIdx.x;
  const int F = pn_counted_frames(lens[b], N, T);
  const size_t row = (size_t)b * T;
  for (int i = lane; i < FV_ROW; i += SA_WAVE) lgt[i] = log_q[i];
  __syncthreads();
  const long long lg_min = lgt[PN_TMIN];

  long long delta = FV_INF;              // lanes past the states stay absent
  int lg_prev = 0;
  for (int c0 = 0; c0 < F; c0 += FV_CHUNK) {
    const int n = min(FV_CHUNK, F - c0);
    for (int i = lane; i < n * FV_K; i += SA_WAVE) {
      const int tau = fv_lag(cand_tau[(row + c0) * FV_K + i]);
      const int q = min(max(cand_q[(row + c0) * FV_K + i], 0), FV_ONE);
      const int lg = lgt[tau < 0 ? 0 : tau];
      c_tau[i] = tau;
      c_lg[i] = lg;
      c_loc[i] = (long long)q + ((bq * ((long long)lg - lg_min)) >> FV_FRAC);
    }
    __syncthreads();
    for (int i = 0; i < n; ++i) {
      const int slot = i * FV_K + (lane < FV_K ? lane : 0);
      const bool present = lane < FV_K ? c_tau[slot] >= 0 : lane == FV_K;
      const long long local = lane < FV_K ? c_loc[slot] : vq;
      const int lg = lane < FV_K ? c_lg[slot] : 0;
      long long best = 0;
      int arg = 0;
      if (c0 + i > 0) {
        best = FV_INF;
#pragma unroll
        for (int a = 0; a < FV_K; ++a) {                     // from a candidate: |LOG difference| < 2^32, j_q < 2^19
          const long long da = fv_from(delta, a);
          const int la = fv_from(lg_prev, a);
          const unsigned diff = (unsigned)max(la, lg) - (unsigned)min(la, lg);
          const long long jump = (long long)(((unsigned long long)jq * diff) >> FV_FRAC);
          const long long c = da + (lane == FV_K ? (long long)sq : jump);
          if (c < best) {                                    // (an absent predecessor's c is at least FV_INF)
            best = c;
            arg = a;
          }
        }
        const long long c = fv_from(delta, FV_K) + (lane == FV_K ? 0LL : (long long)sq);     // from unvoiced
        if (c < best) {
          best = c;
          arg = FV_K;
        }
      }
      delta = present ? local + best : FV_INF;
      lg_prev = lg;
      if (lane < FV_S) c_psi[i * FV_S + lane] = (unsigned char)arg;
    }
    __syncthreads();
    for (int i = lane; i < n * FV_S; i += SA_WAVE) psi[(row + c0) * FV_S + i] = c_psi[i];
    __syncthreads();
  }

  // the cheapest final state, the smaller index on a tie
  long long best = FV_INF;
  int state = FV_K;
#pragma unroll
  for (int a = FV_S - 1; a >= 0; --a) {
    const long long da = fv_from(delta, a);
    if (da <= best && da < FV_INF) {
      best = da;
      state = a;
    }
  }
  __threadfence_block();
  __syncthreads();

  for (int c0 = ((F - 1) / FV_CHUNK) * FV_CHUNK; c0 >= 0; c0 -= FV_CHUNK) {
    const int n = min(FV_CHUNK, F - c0);
    for (int i = lane; i < n * FV_S; i += SA_WAVE) c_psi[i] = psi[(row + c0) * FV_S + i];
    __syncthreads();
    for (int i = n - 1; i >= 0; --i) {
      if (lane == 0) c_path[i] = state < FV_K ? state : -1;
      state = min((int)c_psi[i * FV_S + state], FV_S - 1);
    }
    __syncthreads();
    for (int i = lane; i < n; i += SA_WAVE) {
      const int t = c0 + i, p = c_path[i];
      float hz = 0.0f;
      if (p >= 0) {
        const int tau = fv_lag(cand_tau[(row + t) * FV_K + p]);
        if (tau >= 0) {
          const float* d = dprime + (row + t) * FV_ROW;
          hz = pn_refined_hz(tau, d[tau - 1], d[tau], d[tau + 1]);
        }
      }
      path[row + t] = p;
      f0[row + t] = hz;
    }
    __syncthreads();
  }
  for (int t = F + lane; t < T; t += SA_WAVE) {
    path[row + t] = -1;
    f0[row + t] = 0.0f;
  }
}

static bool fv_weight(float w, long long* q) {
  if (!(w >= 0.0f && w <= 4.0f)) return false;                         // (NaN fails both)
  *q = (long long)(int)lrint(w * (float)FV_ONE);
  return true;
}

extern "C" int sa_f0_viterbi(const float* dprime, const int* cand_tau, const int* cand_q, const float* lens,
                             const int* log_q, int B, int T, int N, float voicing_cost, float switch_cost,
                             float jump_cost, float lag_bias, unsigned char* psi, int* path, float* f0,
                             void* stream) {
  long long vq, sq, jq, bq;
  if (!dprime || !cand_tau || !cand_q || !lens || !log_q || !psi || !path || !f0 || !pn_rows_ok(B) ||
      !pn_frames_ok(T, 1) || !pn_samples_ok(N) || !fv_weight(voicing_cost, &vq) || !fv_weight(switch_cost, &sq) ||
      !fv_weight(jump_cost, &jq) || !fv_weight(lag_bias, &bq))
    return -EINVAL;
  hipLaunchKernelGGL(sa_f0_viterbi_kernel, dim3(B), dim3(SA_WAVE), 0, (hipStream_t)stream, dprime, cand_tau, cand_q,
                     lens, log_q, T, N, vq, (unsigned)sq, (unsigned)jq, bq, psi, path, f0);
  return -(int)hipGetLastError();
}
