// The arithmetic of torch.optim.Adam(fused=True).step() for fp32 tensors, as ONE launch over every
// parameter of a param group.
//
// torch owns the optimizer: param_groups, the state tensors (step, exp_avg, exp_avg_sq), state_dict and the
// learning rate stay where they are, and torch's own step() is the path for every configuration this kernel
// does not cover (ops.adam_step says which).  torch's _fused_adam_ hands each 65 536-element chunk of a tensor
// to one 512-thread block of multi_tensor_apply -- 66 blocks for the ConvAE's 56 tensors / 533 123 parameters,
// each walking up to 32 dependent load -> fp64 math -> store rounds, 89 us as the unoverlapped tail of the
// train step.  Here a block owns SA_ADAM_CHUNK = 1 024 elements of one tensor (one 16-byte access per thread
// and operand), ~580 blocks that are all resident at once.
//
// The update rule is the one of ATen/native/cuda/fused_adam_utils.cuh (torch 2.10) for scalar_type = float,
// ADAM_MODE::ORIGINAL, amsgrad = false, weight_decay = 0, maximize = false, no grad scaler -- and, operation by
// operation, what torch's gfx950 build of it executes, so that the parameters and both moments come out with
// torch's bits:
//   m' = float(fma(beta1, double(m), (1 - beta1) * double(g)))
//   v' = float(fma(beta2, double(v), ((1 - beta2) * double(g)) * double(g)))
//   bc1 = float(1 - pow(beta1, double(step))),  bc2s = float(sqrt(1 - pow(beta2, double(step))))      (fp64, narrowed)
//   step_size = float(lr / double(bc1))                                                                (fp64 division)
//   denom = float(double(sqrtf(v') / bc2s) + eps)
//   p' = p - (step_size * m') / denom                                                                  (fp32, IEEE / and sqrt)
// (the source writes beta * m + (1 - beta) * g in double; torch's build contracts the first product into the
// sum.)  The contractions are spelled out and contraction is off for the rest, so the bits do not depend on
// what a compiler release chooses to fuse.  The step counters are NOT advanced here: torch's _foreach_add_
// stays the caller's first launch (bumping them per block would race between the blocks of one tensor).
#include "sa_common.h"

struct SaAdamCoef { double b1, b2, omb1, omb2, eps; float step_size, bc2s; };

__device__ static inline void sa_adam_math(const SaAdamCoef& k, float g, float& p, float& m, float& v) {
#pragma clang fp contract(off)
  const double gd = (double)g;
  m = (float)fma(k.b1, (double)m, k.omb1 * gd);
  v = (float)fma(k.b2, (double)v, (k.omb2 * gd) * gd);
  const float denom = (float)((double)(sqrtf(v) / k.bc2s) + k.eps);
  p = p - (k.step_size * m) / denom;
}

__global__ __launch_bounds__(256) void sa_adam_kernel(const SaAdamRec* __restrict__ table, int ntensors,
                                                      const int* __restrict__ map, SaFlats bases,
                                                      const float* __restrict__ lr_dev, double lr, double beta1,
                                                      double beta2, double eps) {
#pragma clang fp contract(off)
  const int t = map[2 * blockIdx.x], chunk = map[2 * blockIdx.x + 1];
  if (t < 0 || t >= ntensors || chunk < 0) return;                    // (uniform per workgroup)
  const SaAdamRec r = table[t];
  const long long i0 = (long long)chunk * SA_ADAM_CHUNK + 4 * (long long)threadIdx.x;
  if (i0 >= r.n || r.gbase >= bases.n) return;
  const float* gp = r.gbase >= 0 ? bases.f[r.gbase].p + r.goff : r.g;
  const double step = (double)*r.step;
  const double lrd = lr_dev ? (double)*lr_dev : lr;
  SaAdamCoef k;
  k.b1 = beta1; k.b2 = beta2; k.eps = eps;
  k.omb1 = 1.0 - beta1; k.omb2 = 1.0 - beta2;
  const float bc1 = (float)(1.0 - pow(beta1, step));
  k.bc2s = (float)sqrt(1.0 - pow(beta2, step));
  k.step_size = (float)(lrd / (double)bc1);
  float* pp = r.p + i0; float* mp = r.m + i0; float* vp = r.v + i0; gp += i0;
  const bool vec = i0 + 4 <= r.n &&
                   ((((uintptr_t)pp) | ((uintptr_t)mp) | ((uintptr_t)vp) | ((uintptr_t)gp)) & 15) == 0;
  if (vec) {
    float4 p4 = *reinterpret_cast<const float4*>(pp), m4 = *reinterpret_cast<const float4*>(mp);
    float4 v4 = *reinterpret_cast<const float4*>(vp);
    const float4 g4 = *reinterpret_cast<const float4*>(gp);
    sa_adam_math(k, g4.x, p4.x, m4.x, v4.x);
    sa_adam_math(k, g4.y, p4.y, m4.y, v4.y);
    sa_adam_math(k, g4.z, p4.z, m4.z, v4.z);
    sa_adam_math(k, g4.w, p4.w, m4.w, v4.w);
    *reinterpret_cast<float4*>(pp) = p4;
    *reinterpret_cast<float4*>(mp) = m4;
    *reinterpret_cast<float4*>(vp) = v4;
  } else {
    const int cnt = r.n - i0 < 4 ? (int)(r.n - i0) : 4;
    for (int j = 0; j < cnt; ++j) {
      float p = pp[j], m = mp[j], v = vp[j];
      sa_adam_math(k, gp[j], p, m, v);
      pp[j] = p; mp[j] = m; vp[j] = v;
    }
  }
}

extern "C" int sa_adam_record_bytes(void) { return (int)sizeof(SaAdamRec); }

extern "C" int sa_adam_step(const SaAdamRec* table, int ntensors, const int* map, int nblocks, const SaFlats* bases,
                            const float* lr_dev, double lr, double beta1, double beta2, double eps, void* stream) {
  if (!table || !map || !bases || ntensors <= 0 || nblocks <= 0 || bases->n < 0 || bases->n > SA_FLATS_MAX) return -22;
  for (int j = 0; j < bases->n; ++j)
    if (!bases->f[j].p) return -22;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sa_adam_kernel, dim3(nblocks), dim3(256), 0, st, table, ntensors, map, *bases, lr_dev, lr, beta1,
                     beta2, eps);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : -(int)e;
}
