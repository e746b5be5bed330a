// TD-PSOLA pitch modification (pitchnorm.PitchNormalizer(psola=True)): the waveform is cut into
// two-period grains centred on pitch marks and the same grains are laid down again at the new spacing.  No STFT, no
// phase, no iteration, no random number; the spectral envelope stays where it was and the duration is kept.
//   sa_psola_marks   wav, f0 -> the analysis marks of every row: a serial chain of windowed argmaxes, one wave per row
//   sa_psola_plan    marks, rho_q -> where every grain goes (syn_pos) and which mark it is cut at (syn_src)
//   sa_psola_ola     the overlap-add in gather form: every output sample sums the grains that reach it, in ascending j
// Every decision is made on integers, or on fp64 formed from the fp32 inputs (include/sa_hip.h states the algorithm).
// Plain HIP C++, no atomics, fixed summation orders: the same bits on every run.
#include "sa_common.h"
#include "sa_pitch_shared.h"
#include <errno.h>
#include <limits.h>
#include <math.h>

#define PS_U 80                          // mark spacing where the frame is unvoiced
#define PS_SMIN 30                       // mark spacing: tau_min - tau_min / 4 ..
#define PS_SMAX 332                      // .. tau_max + tau_max / 4
#define PS_MDIV 30                       // Mcap = N / 30 + 2
#define PS_JDIV 15                       // Jcap = N / 15 + 2: a grain every P / 2 samples at the least
#define PS_MAX_N (1 << 24)
#define PS_CHUNK 4096                    // samples per staged chunk of sa_psola_marks
#define PS_FR (PS_CHUNK / PN_HOP + 3)    // the periods of the frames a chunk's samples lie in
#define PS_PCHUNK 1024                   // marks per staged chunk of sa_psola_plan
#define PS_TILE 256                      // samples per workgroup of sa_psola_ola
#define PS_G 64                          // grains staged per tile: (256 + 2 * 332) / 15 + 1 = 62 can reach one
#define PS_RHO_ONE (1 << 16)

extern "C" int sa_psola_dim(int which) {
  switch (which) {
    case 0: return PS_U;
    case 1: return PN_TMIN;
    case 2: return PN_TMAX;
    case 3: return PS_SMIN;
    case 4: return PS_SMAX;
    case 5: return PS_TILE;
    case 6: return PS_MDIV;
    case 7: return PS_JDIV;
    default: return -EINVAL;
  }
}

extern "C" long long sa_psola_workspace_bytes(int B, int N) {
  if (!pn_rows_ok(B) || N < 1 || N > PS_MAX_N) return -EINVAL;
  return 8LL * (long long)B * (long long)(N / PS_MDIV + 2);
}

static inline bool ps_frames_ok(int N, int T) { return T == N / PN_HOP + 1 || T == (N + PN_HOP - 1) / PN_HOP + 1; }

__device__ static inline int ps_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ static inline int ps_frame(int n, int T) { return min((n + PN_HOP / 2) / PN_HOP, T - 1); }
__device__ static inline int ps_counted(int nv, int T) { return min(T, nv / PN_HOP + 1); }

// per[t]: the period of frame t in samples, 0 where it is unvoiced or does not count (a NaN is unvoiced)
__device__ static inline int ps_period(const float* __restrict__ f0, int t, int F) {
  if (t >= F) return 0;
  const float f = f0[t];
  if (!(f > 0.0f)) return 0;
  return (int)fmin(fmax(rint(16000.0 / (double)f), (double)PN_TMIN), (double)PN_TMAX);
}

// ---- marks -------------------------------------------------------------------------------------------
// The argmax as a maximum of integer keys: the sample as an unsigned whose order is the floats' (-0 staged as +0, a
// NaN as -inf) in the high word, PS_IDX_TOP - index in the low one, so that the larger value wins and on a tie the
// smaller index.
#define PS_IDX_TOP 0x7fffffffu

__device__ static inline unsigned ps_ordered(float v) {
  const unsigned u = __float_as_uint(v);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ static inline unsigned long long ps_key(float v, int i) {
  return ((unsigned long long)ps_ordered(v) << 32) | (unsigned long long)(PS_IDX_TOP - (unsigned)i);
}

// the maximum with the lane a DPP pattern names: a move within the row of 16 lanes, no trip through LDS.  Every
// pattern used is a permutation of the row and all 64 lanes are active, so every lane reads a live one.
template <int CTRL>
__device__ static inline unsigned long long ps_row_max(unsigned long long k) {
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(k >> 32), CTRL, 0xf, 0xf, false);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)k, CTRL, 0xf, 0xf, false);
  return max(k, ((unsigned long long)hi << 32) | (unsigned long long)lo);
}

__device__ static inline unsigned long long ps_lane_key(unsigned long long k, int lane) {
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(k >> 32), lane);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)k, lane);
  return ((unsigned long long)hi << 32) | (unsigned long long)lo;
}

// The argmax of the staged samples lo..hi (xs holds them from c0 on), hi - lo < 64 Q, in every lane: Q reads per lane
// that go out together (one past hi reads hi again), the keys reduced within each row of 16 lanes by four DPP steps and
// across the four rows by lane reads.
template <int Q>
__device__ static inline int ps_argmax(const float* xs, int c0, int lo, int hi, int lane) {
  unsigned long long key = 0ull;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = min(lo + lane + q * SA_WAVE, hi);
    key = max(key, ps_key(xs[i - c0], i));
  }
  key = ps_row_max<0xB1>(key);                                // lanes ^ 1, ^ 2 (quad_perm), then the other quad
  key = ps_row_max<0x4E>(key);                                // (row_half_mirror) and the other half (row_mirror) of
  key = ps_row_max<0x141>(key);                               // the row of 16
  key = ps_row_max<0x140>(key);
  key = max(max(ps_lane_key(key, 0), ps_lane_key(key, 16)), max(ps_lane_key(key, 32), ps_lane_key(key, 48)));
  return (int)(PS_IDX_TOP - (unsigned)key);
}

#define PS_Q_FIRST ((PN_TMAX + SA_WAVE - 1) / SA_WAVE)                   // the first window: a whole period, up to 266 samples
#define PS_Q_NEXT ((2 * (PN_TMAX / 4) + 1 + SA_WAVE - 1) / SA_WAVE)      // every later one: p / 4 either side, up to 133

// grid (B), one wave per row.  The wave stages PS_CHUNK samples from the window's first sample on and the periods of
// the frames those samples lie in.  The first window is the first period, at most 266 samples, five per lane; every
// later one is at most 133 samples, three per lane.  The chunk is staged again when a window ends past it: about once
// in 4096 / 332 = 12 steps at the least.
__global__ __launch_bounds__(SA_WAVE) void sa_psola_marks_kernel(const float* __restrict__ wav,
                                                                 const float* __restrict__ f0g,
                                                                 const int* __restrict__ n_valid, int N, int T,
                                                                 int Mcap, int* __restrict__ marks,
                                                                 int* __restrict__ count) {
  __shared__ float xs[PS_CHUNK];
  __shared__ int pf[PS_FR];
  const int lane = threadIdx.x, b = blockIdx.x;
  const int nv = ps_clamp(n_valid[b], 0, N), F = ps_counted(nv, T);
  const float* x = wav + (size_t)b * N;
  const float* f0 = f0g + (size_t)b * T;
  int* mk = marks + (size_t)b * Mcap;

  int c0 = -1, fb = 0, k = 0;
  int lo = 0, hi = 0;
  {
    const int p = ps_period(f0, 0, F);
    hi = p > 0 ? p - 1 : 0;
  }
  while (hi < nv && k < Mcap) {
    if (c0 < 0 || hi >= c0 + PS_CHUNK) {
      __syncthreads();
      c0 = lo;
      fb = ps_frame(c0, T);
#pragma unroll 16
      for (int q = 0; q < PS_CHUNK / SA_WAVE; ++q) {            // (branch-free, so that the loads go out in batches)
        const int i = q * SA_WAVE + lane, s = c0 + i;
        const float v = x[min(s, nv - 1)];                      // (hi < nv: the row has a sample)
        xs[i] = (s >= nv || v != v) ? -INFINITY : (v == 0.0f ? 0.0f : v);
      }
      for (int i = lane; i < PS_FR; i += SA_WAVE) pf[i] = fb + i < T ? ps_period(f0, fb + i, F) : 0;
      __syncthreads();
    }
    int m = lo;
    if (hi > lo)                                              // (the same in every lane, and so is k)
      m = k == 0 ? ps_argmax<PS_Q_FIRST>(xs, c0, lo, hi, lane) : ps_argmax<PS_Q_NEXT>(xs, c0, lo, hi, lane);
    if (lane == 0) mk[k] = m;
    ++k;
    const int p = pf[min(ps_frame(m, T) - fb, PS_FR - 1)];
    if (p > 0) {
      lo = m + p - (p >> 2);
      hi = m + p + (p >> 2);
    } else {
      lo = hi = m + PS_U;
    }
  }
  if (lane == 0) count[b] = k;
}

extern "C" int sa_psola_marks(const float* wav, const float* f0, const int* n_valid, int B, int N, int T, int* marks,
                              int* count, void* stream) {
  if (!wav || !f0 || !n_valid || !marks || !count || !pn_rows_ok(B) || N < 1 || N > PS_MAX_N || !ps_frames_ok(N, T))
    return -EINVAL;
  hipLaunchKernelGGL(sa_psola_marks_kernel, dim3(B), dim3(SA_WAVE), 0, (hipStream_t)stream, wav, f0, n_valid, N, T,
                     N / PS_MDIV + 2, marks, count);
  return -(int)hipGetLastError();
}

// ---- plan --------------------------------------------------------------------------------------------
// grid (B), one wave per row.  First the lanes form, per mark, the step a grain cut there advances the synthesis
// position by (P inv, int64, units of 2^-16 samples) into the caller's workspace: the one 64-bit division is off the
// chain.  Then every lane walks the chain (the same walk: broadcast reads) over marks and steps staged through LDS
// PS_PCHUNK at a time; the nearest-mark pointer only ever advances.  A period is clamped to the spacing bounds and a
// mark to the row, which changes nothing in a table sa_psola_marks wrote and ends the walk for any other.
__global__ __launch_bounds__(SA_WAVE) void sa_psola_plan_kernel(const int* __restrict__ marks,
                                                                const int* __restrict__ count,
                                                                const float* __restrict__ f0g,
                                                                const int* __restrict__ rho_q,
                                                                const int* __restrict__ n_valid, int N, int T,
                                                                int Mcap, int Jcap, long long* stepg,
                                                                int* __restrict__ syn_pos, int* __restrict__ syn_src,
                                                                int* __restrict__ syn_count) {
  __shared__ int sm[PS_PCHUNK];
  __shared__ long long ss[PS_PCHUNK];
  const int lane = threadIdx.x, b = blockIdx.x;
  const int nv = ps_clamp(n_valid[b], 0, N), F = ps_counted(nv, T);
  const int M = ps_clamp(count[b], 0, Mcap);
  const int* mk = marks + (size_t)b * Mcap;
  const float* f0 = f0g + (size_t)b * T;
  const int* rq = rho_q + (size_t)b * T;
  long long* step = stepg + (size_t)b * Mcap;
  int* sp = syn_pos + (size_t)b * Jcap;
  int* sr = syn_src + (size_t)b * Jcap;
  if (M < 2) {
    if (lane == 0) syn_count[b] = 0;
    return;
  }
  for (int a = lane; a < M; a += SA_WAVE) {
    const int ma = ps_clamp(mk[a], 0, N - 1);
    const int P = a + 1 < M ? ps_clamp(mk[a + 1], 0, N - 1) - ma : ma - ps_clamp(mk[a - 1], 0, N - 1);
    const int t = ps_frame(ma, T);
    const long long r = ps_period(f0, t, F) > 0 ? (long long)ps_clamp(rq[t], PS_RHO_ONE / 2, 2 * PS_RHO_ONE)
                                                : (long long)PS_RHO_ONE;
    const long long inv = ((1LL << 32) + r / 2) / r;
    step[a] = (long long)ps_clamp(P, PS_SMIN, PS_SMAX) * inv;
  }
  __syncthreads();

  const long long last = (long long)ps_clamp(mk[M - 1], 0, N - 1) << 16;
  int a0 = 0, a = 0, j = 0;
  for (int i = lane; i < PS_PCHUNK && i < M; i += SA_WAVE) {
    sm[i] = ps_clamp(mk[i], 0, N - 1);
    ss[i] = step[i];
  }
  __syncthreads();
  // the mark the pointer is at, the next one and the step, in registers: the chain waits for LDS only when it advances
  long long mc = (long long)sm[0] << 16, mn = (long long)sm[1] << 16, st = ss[0];
  long long s = mc;
  while (s <= last && j < Jcap) {
    while (a + 1 < M && llabs(mn - s) < llabs(mc - s)) {
      ++a;
      if (a + 1 >= a0 + PS_PCHUNK) {
        __syncthreads();
        a0 = a;
        for (int i = lane; i < PS_PCHUNK && a0 + i < M; i += SA_WAVE) {
          sm[i] = ps_clamp(mk[a0 + i], 0, N - 1);
          ss[i] = step[a0 + i];
        }
        __syncthreads();
      }
      mc = mn;
      mn = a + 1 < M ? (long long)sm[a + 1 - a0] << 16 : mc;
      st = ss[a - a0];
    }
    if (lane == 0) {
      sp[j] = (int)((s + (1LL << 15)) >> 16);
      sr[j] = a;
    }
    s += st;
    ++j;
  }
  if (lane == 0) syn_count[b] = j;
}

extern "C" int sa_psola_plan(const int* marks, const int* count, const float* f0, const int* rho_q,
                             const int* n_valid, int B, int N, int T, void* ws, int* syn_pos, int* syn_src,
                             int* syn_count, void* stream) {
  if (!marks || !count || !f0 || !rho_q || !n_valid || !ws || !syn_pos || !syn_src || !syn_count || !pn_rows_ok(B) ||
      N < 1 || N > PS_MAX_N || !ps_frames_ok(N, T))
    return -EINVAL;
  hipLaunchKernelGGL(sa_psola_plan_kernel, dim3(B), dim3(SA_WAVE), 0, (hipStream_t)stream, marks, count, f0, rho_q,
                     n_valid, N, T, N / PS_MDIV + 2, N / PS_JDIV + 2, (long long*)ws, syn_pos, syn_src, syn_count);
  return -(int)hipGetLastError();
}

// ---- overlap-add -------------------------------------------------------------------------------------
// One grain's share of output sample n = pos + d: the weight (fp64, rounded once) times the source sample m + d, both
// added in fp32 without contraction.  L, R: the half-widths; a negative one is a rectangular side, which only the
// source range ends.
__device__ static inline void ps_add(const float* __restrict__ x, int nv, int d, int m, int L, int R, float* acc,
                                     float* wsum) {
  const int h = d < 0 ? L : R;
  float w = 1.0f;
  if (d != 0 && h >= 0) {
    if (abs(d) >= h) return;
    w = (float)(0.5 * (1.0 + cos(3.14159265358979323846 * (double)d / (double)h)));
  }
  const int i = m + d;
  if (i < 0 || i >= nv) return;
  *acc = __fadd_rn(*acc, __fmul_rn(w, x[i]));
  *wsum = __fadd_rn(*wsum, w);
}

// grain j of a row -> its position, source mark and half-widths; everything read from the tables is clamped
__device__ static inline void ps_grain(const int* __restrict__ mk, const int* __restrict__ sp,
                                       const int* __restrict__ sr, int j, int J, int M, int N, int* pos, int* m,
                                       int* L, int* R) {
  const int a = ps_clamp(sr[j], 0, M - 1);
  const int ma = ps_clamp(mk[a], 0, N - 1);
  const int below = a > 0 ? ma - ps_clamp(mk[a - 1], 0, N - 1) : ps_clamp(mk[1], 0, N - 1) - ma;
  const int above = a + 1 < M ? ps_clamp(mk[a + 1], 0, N - 1) - ma : below;
  *pos = ps_clamp(sp[j], 0, N - 1);
  *m = ma;
  *L = j == 0 ? -1 : ps_clamp(a > 0 ? below : above, PS_SMIN, PS_SMAX);
  *R = j == J - 1 ? -1 : ps_clamp(above, PS_SMIN, PS_SMAX);
}

// grid (tiles of 256 samples, B).  A grain but the last reaches at most 332 samples either way, so the grains that
// can reach the tile are those with n0 - 332 <= syn_pos <= n0 + 255 + 332: two binary searches over syn_pos, at most
// 62 grains (their spacing is 15 at the least), staged in LDS and walked by every lane in ascending j.  The last
// grain's rectangular side reaches as far as the row's samples do; every tile takes it after the staged ones, from
// registers.  The reads of wav[m + d] are contiguous across the lanes.
__global__ __launch_bounds__(PS_TILE) void sa_psola_ola_kernel(const float* __restrict__ wav,
                                                               const int* __restrict__ marks,
                                                               const int* __restrict__ count,
                                                               const int* __restrict__ syn_pos,
                                                               const int* __restrict__ syn_src,
                                                               const int* __restrict__ syn_count,
                                                               const int* __restrict__ n_valid, int N, int Mcap,
                                                               int Jcap, float* __restrict__ out) {
  __shared__ int g_pos[PS_G], g_m[PS_G], g_L[PS_G], g_R[PS_G];
  const int tid = threadIdx.x, b = blockIdx.y, n0 = blockIdx.x * PS_TILE, n = n0 + tid;
  const int nv = ps_clamp(n_valid[b], 0, N);
  const int M = ps_clamp(count[b], 0, Mcap), J = ps_clamp(syn_count[b], 0, Jcap);
  const float* x = wav + (size_t)b * N;
  float* y = out + (size_t)b * N;
  if (M < 2 || J < 1 || n0 >= nv) {                           // (the same in every thread) no plan: a copy
    if (n < N) y[n] = n < nv ? x[n] : 0.0f;
    return;
  }
  const int* mk = marks + (size_t)b * Mcap;
  const int* sp = syn_pos + (size_t)b * Jcap;
  const int* sr = syn_src + (size_t)b * Jcap;

  int lo = 0, hi = J;                                         // the first j with syn_pos[j] >= n0 - 332
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sp[mid] < n0 - PS_SMAX) lo = mid + 1; else hi = mid;
  }
  const int jlo = lo;
  hi = J;                                                     // the first j with syn_pos[j] > n0 + 255 + 332
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sp[mid] <= n0 + PS_TILE - 1 + PS_SMAX) lo = mid + 1; else hi = mid;
  }
  const int ng = max(min(min(lo, J - 1), jlo + PS_G) - jlo, 0);
  if (tid < ng) ps_grain(mk, sp, sr, jlo + tid, J, M, N, &g_pos[tid], &g_m[tid], &g_L[tid], &g_R[tid]);
  int e_pos, e_m, e_L, e_R;
  ps_grain(mk, sp, sr, J - 1, J, M, N, &e_pos, &e_m, &e_L, &e_R);
  __syncthreads();
  if (n >= N) return;
  float acc = 0.0f, wsum = 0.0f;
  if (n < nv) {
    for (int g = 0; g < ng; ++g) ps_add(x, nv, n - g_pos[g], g_m[g], g_L[g], g_R[g], &acc, &wsum);
    ps_add(x, nv, n - e_pos, e_m, e_L, e_R, &acc, &wsum);
    acc = __fdiv_rn(acc, fmaxf(wsum, 0.5f));
  }
  y[n] = acc;
}

extern "C" int sa_psola_ola(const float* wav, const int* marks, const int* count, const int* syn_pos,
                            const int* syn_src, const int* syn_count, const int* n_valid, int B, int N, float* out,
                            void* stream) {
  if (!wav || !marks || !count || !syn_pos || !syn_src || !syn_count || !n_valid || !out || !pn_rows_ok(B) || N < 1 ||
      N > PS_MAX_N)
    return -EINVAL;
  hipLaunchKernelGGL(sa_psola_ola_kernel, dim3(sa_div_up(N, PS_TILE), B), dim3(PS_TILE), 0, (hipStream_t)stream, wav,
                     marks, count, syn_pos, syn_src, syn_count, n_valid, N, N / PS_MDIV + 2, N / PS_JDIV + 2, out);
  return -(int)hipGetLastError();
}
