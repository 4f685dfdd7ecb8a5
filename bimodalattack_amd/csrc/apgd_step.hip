// a5b -- auto-PGD L-inf step (reference bimodal_attack.py:1039-1110, perform_autopgd_step).
//
// The per-pixel part of one call; the host (ops.ApgdState) keeps eta, the losses and the
// counters and passes the two decisions of the call as flags:
//
//   z    = clamp(max(min(x - eta*sign(g), x0+eps), x0-eps), 0, 1)
//   new  = clamp(max(min((x + 0.75*(z-x)) + 0.25*(x-prev), x0+eps), x0-eps), 0, 1)
//   prev = x
//   take_best:  best = new                    (the step loss improved on the best one)
//   restart:    out = prev = best             (a checkpoint halved eta)
//   otherwise:  out = new
//
// With restart and no take_best the kernel reads best only (x, g, x0, prev are not touched).
// HBM-bound streaming, no reductions: 16 B read (x, g, x0, prev) + 8 B written (out, prev)
// per pixel, + 4 B when best is written.  Same launch shape as linf_step.hip: one float4 per
// lane per access, grid-stride over <= 2048 workgroups, a scalar kernel for the tail.
//
// Bit-exactness notes: sign() is torch's ((g>0) - (g<0): 0 for NaN and -0.0); eta*sign is
// exact.  torch.min / torch.max propagate a NaN from either operand and return the FIRST
// operand on a tie (+-0), unlike linf_one's compare+select; clamp(0, 1) is compare+select
// (keeps -0.0, propagates NaN).  The momentum line is rounded op by op in fp32 as the
// reference evaluates it, so FMA contraction is off in apgd_one.

#include "bma_common.h"
#include "bma_profile.h"

namespace {

__device__ __forceinline__ float torch_min(float a, float b) {
  if (a != a) return a;
  if (b != b) return b;
  return b < a ? b : a;
}

__device__ __forceinline__ float torch_max(float a, float b) {
  if (a != a) return a;
  if (b != b) return b;
  return a < b ? b : a;
}

__device__ __forceinline__ float clamp01(float y) {
  y = y < 0.0f ? 0.0f : y;
  return y > 1.0f ? 1.0f : y;
}

__device__ __forceinline__ float apgd_one(float x, float g, float x0, float prev, float eps, float eta) {
#pragma clang fp contract(off)
  const float s = (g > 0.0f ? 1.0f : 0.0f) - (g < 0.0f ? 1.0f : 0.0f);
  const float hi = x0 + eps, lo = x0 - eps;
  const float z = clamp01(torch_max(torch_min(x - eta * s, hi), lo));
  const float a = 0.75f * (z - x);
  const float b = 0.25f * (x - prev);
  const float m = (x + a) + b;
  return clamp01(torch_max(torch_min(m, hi), lo));
}

__global__ __launch_bounds__(256) void apgd_step_vec4(const bma::float4_t* x, const bma::float4_t* __restrict__ g,
                                                      const bma::float4_t* __restrict__ x0, bma::float4_t* __restrict__ prev,
                                                      bma::float4_t* __restrict__ best, bma::float4_t* out, int64_t n4,
                                                      float eps, float eta, int take_best, int restart) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n4; i += stride) {
    if (restart && !take_best) {
      const bma::float4_t vb = best[i];
      prev[i] = vb;
      out[i] = vb;
      continue;
    }
    const bma::float4_t vx = x[i], vg = g[i], v0 = x0[i], vp = prev[i];
    bma::float4_t r;
    r.x = apgd_one(vx.x, vg.x, v0.x, vp.x, eps, eta);
    r.y = apgd_one(vx.y, vg.y, v0.y, vp.y, eps, eta);
    r.z = apgd_one(vx.z, vg.z, v0.z, vp.z, eps, eta);
    r.w = apgd_one(vx.w, vg.w, v0.w, vp.w, eps, eta);
    if (take_best) best[i] = r;
    prev[i] = restart ? r : vx;
    out[i] = r;
  }
}

__global__ __launch_bounds__(256) void apgd_step_scalar(const float* x, const float* g, const float* x0, float* prev,
                                                        float* best, float* out, int64_t begin, int64_t n, float eps,
                                                        float eta, int take_best, int restart) {
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = begin + static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (restart && !take_best) {
      const float vb = best[i];
      prev[i] = vb;
      out[i] = vb;
      continue;
    }
    const float vx = x[i];
    const float r = apgd_one(vx, g[i], x0[i], prev[i], eps, eta);
    if (take_best) best[i] = r;
    prev[i] = restart ? r : vx;
    out[i] = r;
  }
}

}  // namespace

extern "C" int bma_apgd_step(const float* x, const float* g, const float* x0, float* prev, float* best, int64_t n,
                             float eps, float eta, int take_best, int restart, float* out, void* stream) {
  if (n < 0 || (n > 0 && (!x || !g || !x0 || !prev || !best || !out))) return BMA_EINVAL;
  if ((take_best != 0 && take_best != 1) || (restart != 0 && restart != 1)) return BMA_EINVAL;
  if (n > 0 && (prev == best || prev == x || prev == out || best == x || best == out)) return BMA_EINVAL;
  if (n == 0) return BMA_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g) |
                         reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(prev) |
                         reinterpret_cast<uintptr_t>(best) | reinterpret_cast<uintptr_t>(out);
  if (bits & 3) return BMA_EALIGN;
  int64_t done = 0;
  if ((bits & 15) == 0 && n >= 4) {
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    const double px_bytes = (restart && !take_best) ? 12.0 : (take_best ? 28.0 : 24.0);
    BMA_PROF_BEGIN(BMA_K_APGD, st, px_bytes * static_cast<double>(n4) * 4.0);
    hipLaunchKernelGGL(apgd_step_vec4, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, st,
                       reinterpret_cast<const bma::float4_t*>(x), reinterpret_cast<const bma::float4_t*>(g),
                       reinterpret_cast<const bma::float4_t*>(x0), reinterpret_cast<bma::float4_t*>(prev),
                       reinterpret_cast<bma::float4_t*>(best), reinterpret_cast<bma::float4_t*>(out), n4, eps, eta,
                       take_best, restart);
    BMA_PROF_END(BMA_K_APGD, st);
    BMA_LAUNCH_CHECK();
    done = n4 * 4;
  }
  if (done < n) {
    int64_t blocks = (n - done + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(apgd_step_scalar, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, st, x, g, x0, prev, best,
                       out, done, n, eps, eta, take_best, restart);
    BMA_LAUNCH_CHECK();
  }
  return BMA_OK;
}
