// McAdams-coefficient anonymisation (mcadams.py): per frame of 320 samples at hop 160 under the
// periodic sqrt-Hann window, an order-20 LPC fit, every complex pole's angle phi raised to the power alpha, and the
// frame re-synthesised from its own residual; then overlap-add and RMS level matching.  Steps in fp64, the frame
// store and the output in fp32:
//   f = w x;  r_k = sum_j f[j] f[j + k];  r_0 < 1e-10: silent (status 1), rec = f;  r_0 *= 1 + 1e-9
//   a = Levinson-Durbin(r);  some |k_i| >= 1 or an error <= 0: fallback (status 2), rec = f
//   z = the 20 roots of a by Aberth-Ehrlich, one lane per root, at most 64 iterations, stop under 1e-14
//   a' = prod_{real}(1 - Re z x) prod_{Im z > 0}(1 - 2 |z| cos(phi^alpha) x + |z|^2 x^2);  a count that does not add
//        up to 20 or no convergence: fallback
//   res = FIR(a) f;  rec = IIR(1 / a') res;  F_t = fp32(rec w)
//   y[n] = F_t0[n - 160 t0 + 160] + F_{t0 + 1}[n - 160 t0], t0 = n / 160 (a gather);  out = fp32(g y)
// The kernels are sa_lpc_shared.h's, which sa_pole_warp and sa_srcfilt_synth share: this file says what McAdams does
// to a pole's angle.  No atomics, every sum in a fixed order: the same bits on every run.
#include "sa_lpc_shared.h"

extern "C" int sa_mcadams_dim(int which) {
  switch (which) {
    case 0: return SA_FR_W;
    case 1: return SA_FR_H;
    case 2: return SA_FR_P;
    case 3: return SA_FR_G;
    case 4: return SA_FR_THREADS;
    case 5: return SA_LPC_ITERS;
    case 6: return SA_FR_CHUNK;
    default: return -EINVAL;
  }
}

struct SaMcAdamsMap {
  static constexpr bool COPIES = true;                      // alpha = 1: the row is copied and no frame is read
  __device__ static inline double clamp(float a) {          // a coefficient no kernel can be led astray by
    return a >= 0.25f && a <= 2.0f ? (double)a : (a > 2.0f ? 2.0 : (a < 0.25f ? 0.25 : 1.0));
  }
  __device__ static inline double angle(double phi, double al) { return pow(phi, al); }
};

extern "C" int sa_mcadams(const float* wav, const float* alpha, const int* n_valid, int B, int N, int level,
                          float* out, void* ws, int* status, float* gain, void* stream) {
  return sa_fr_roots<SaMcAdamsMap>(wav, alpha, n_valid, B, N, level, out, ws, status, gain, stream);
}
