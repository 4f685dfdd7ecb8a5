// a5c -- PGD image update in the L2 ball (opt-in, EngineOptions.pgd_norm = "l2"; the reference has
// no L2 update).  The arithmetic contract is in include/bma.h next to the entry points:
//
//   nrm(v) = float( sqrt( sum_i double(v_i)^2 ) )            fp64 accumulation, rounded once
//   P(y)   = clamp01( x0 + (y - x0) * min(eps / nrm(y - x0), 1) )
//   u      = g / (nrm(g) + 1e-10f)
//   plain:     out = P(x - step*u)
//   auto-PGD:  z = P(x - eta*u);  m = (x + 0.75*(z - x)) + 0.25*(x - prev);  new = P(m)
//              prev / best / take_best / restart as bma_apgd_step
//
// Unlike linf_step.hip and apgd_step.hip this is not one streaming launch: every norm is a
// reduction over the whole image that the next expression depends on.  The call is a chain of
// ordinary launches on the caller's stream (no cooperative grid, no flag anybody waits on):
//
//   pass 1   sum g^2                                          -> part A            4 B / pixel
//   pass 2   ng = nrm from A;  y = x - step*u;  sum (y-x0)^2  -> part B, norms[0]  12 B / pixel
//   plain    pass 3   nd from B;  out = P(y)                  -> out, norms[1]     16 B / pixel
//   auto-PGD pass 3   nd from B;  z, m;  sum (m-x0)^2         -> part C, norms[1]  16 B / pixel
//            pass 4   nm from C;  new = P(m); prev, best, out -> norms[2]          24-28 B / pixel
//
// Later passes recompute the cheap per-pixel expressions (u, y, z, m) from the inputs instead of
// storing them; a finished norm is handed on as the fp32 value in `norms` (a launch boundary
// orders the write before the read), so each pass adds up one set of partials only.
//
// Reduction data flow, all of it in a fixed order (two runs on one input are bitwise equal, no
// floating-point atomics): a lane accumulates its grid-stride elements in fp64, a wave64 xor
// butterfly, the 16 wave sums through LDS added by thread 0 in wave order, ONE fp64 partial per
// workgroup in ws.  The consuming launch adds the partials in index order (thread 0, once per
// workgroup).  That serial chain is why the grid is at most 256 workgroups of 1024 lanes (one
// per CU, 16 waves each) rather than linf_step's 2048 x 256: 256 dependent fp64 adds instead of 2048.
//
// Vector / tail split as in linf_step.hip: float4 per lane when every pointer is 16-byte aligned,
// the last n % 4 pixels (or all of them when a pointer is not) through the scalar loop of the same
// launch, so a workgroup's partial covers both.
//
// Bit-exactness: FMA contraction is off (every fp32 operation rounds as the torch restatement's
// ops round), fp32 division is the IEEE-rounded one (the build has no fast-math), clamp01 is
// compare+select (keeps -0.0, propagates NaN), min(eps/nrm, 1) propagates NaN like torch.minimum.

#include "bma_common.h"
#include "bma_profile.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / BMA_WAVE;
constexpr int kMaxBlocks = 256;

__device__ __forceinline__ float clamp01(float y) {
  y = y < 0.0f ? 0.0f : y;
  return y > 1.0f ? 1.0f : y;
}

// min(eps / nrm, 1) with torch.minimum's NaN rule; a zero norm gives inf, so 1
__device__ __forceinline__ float ball_factor(float eps, float nrm) {
  const float q = eps / nrm;
  if (q != q) return q;
  return q < 1.0f ? q : 1.0f;
}

__device__ __forceinline__ float descent(float x, float g, float den, float step) {
#pragma clang fp contract(off)
  const float u = g / den;
  const float t = step * u;
  return x - t;
}

__device__ __forceinline__ float project(float y, float x0, float f) {
#pragma clang fp contract(off)
  const float d = y - x0;
  const float p = d * f;
  return clamp01(x0 + p);
}

__device__ __forceinline__ float momentum(float x, float z, float prev) {
#pragma clang fp contract(off)
  const float a = 0.75f * (z - x);
  const float b = 0.25f * (x - prev);
  return (x + a) + b;
}

__device__ __forceinline__ double sq(float v) {
  const double d = static_cast<double>(v);
  return d * d;
}

// this workgroup's partial -> part[blockIdx.x]
__device__ __forceinline__ void store_partial(double acc, double* part) {
  __shared__ double wave_sums[kWaves];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, BMA_WAVE);
  if ((threadIdx.x & (BMA_WAVE - 1)) == 0) wave_sums[threadIdx.x / BMA_WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += wave_sums[w];
    part[blockIdx.x] = s;
  }
}

// float(sqrt(part[0] + part[1] + ...)) in index order, the same value in every lane
__device__ __forceinline__ float norm_from(const double* part, int nb) {
  __shared__ double total;
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < nb; ++i) s += part[i];
    total = s;
  }
  __syncthreads();
  return static_cast<float>(sqrt(total));
}

#define L2_GRID_BEGIN const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x; \
                      const int64_t first = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x

__global__ __launch_bounds__(kThreads) void l2_sumsq_g(const float* __restrict__ g, int64_t n4, int64_t n,
                                                       double* __restrict__ part) {
  L2_GRID_BEGIN;
  double acc = 0.0;
  const bma::float4_t* g4 = reinterpret_cast<const bma::float4_t*>(g);
  for (int64_t i = first; i < n4; i += stride) {
    const bma::float4_t v = g4[i];
    acc += sq(v.x);
    acc += sq(v.y);
    acc += sq(v.z);
    acc += sq(v.w);
  }
  for (int64_t i = n4 * 4 + first; i < n; i += stride) acc += sq(g[i]);
  store_partial(acc, part);
}

// pass 2 of both rules: y = x - step*u, sum (y - x0)^2
__global__ __launch_bounds__(kThreads) void l2_sumsq_y(const float* __restrict__ x, const float* __restrict__ g,
                                                       const float* __restrict__ x0, int64_t n4, int64_t n, float step,
                                                       const double* __restrict__ part_g, int nb,
                                                       double* __restrict__ part_y, float* __restrict__ norms) {
#pragma clang fp contract(off)
  L2_GRID_BEGIN;
  const float ng = norm_from(part_g, nb);
  if (first == 0) norms[0] = ng;
  const float den = ng + 1e-10f;
  double acc = 0.0;
  const bma::float4_t* x4 = reinterpret_cast<const bma::float4_t*>(x);
  const bma::float4_t* g4 = reinterpret_cast<const bma::float4_t*>(g);
  const bma::float4_t* o4 = reinterpret_cast<const bma::float4_t*>(x0);
  for (int64_t i = first; i < n4; i += stride) {
    const bma::float4_t vx = x4[i], vg = g4[i], v0 = o4[i];
    acc += sq(descent(vx.x, vg.x, den, step) - v0.x);
    acc += sq(descent(vx.y, vg.y, den, step) - v0.y);
    acc += sq(descent(vx.z, vg.z, den, step) - v0.z);
    acc += sq(descent(vx.w, vg.w, den, step) - v0.w);
  }
  for (int64_t i = n4 * 4 + first; i < n; i += stride) acc += sq(descent(x[i], g[i], den, step) - x0[i]);
  store_partial(acc, part_y);
}

// pass 3 of the plain step: out = P(y).  out may alias x (each lane reads its pixel before it writes it).
__global__ __launch_bounds__(kThreads) void l2_apply(const float* x, const float* __restrict__ g,
                                                     const float* __restrict__ x0, float* out, int64_t n4, int64_t n,
                                                     float eps, float step, const double* __restrict__ part_y, int nb,
                                                     float* norms) {
  L2_GRID_BEGIN;
  const float den = norms[0] + 1e-10f;
  const float nd = norm_from(part_y, nb);
  if (first == 0) norms[1] = nd;
  const float f = ball_factor(eps, nd);
  const bma::float4_t* x4 = reinterpret_cast<const bma::float4_t*>(x);
  const bma::float4_t* g4 = reinterpret_cast<const bma::float4_t*>(g);
  const bma::float4_t* o4 = reinterpret_cast<const bma::float4_t*>(x0);
  bma::float4_t* r4 = reinterpret_cast<bma::float4_t*>(out);
  for (int64_t i = first; i < n4; i += stride) {
    const bma::float4_t vx = x4[i], vg = g4[i], v0 = o4[i];
    bma::float4_t r;
    r.x = project(descent(vx.x, vg.x, den, step), v0.x, f);
    r.y = project(descent(vx.y, vg.y, den, step), v0.y, f);
    r.z = project(descent(vx.z, vg.z, den, step), v0.z, f);
    r.w = project(descent(vx.w, vg.w, den, step), v0.w, f);
    r4[i] = r;
  }
  for (int64_t i = n4 * 4 + first; i < n; i += stride) out[i] = project(descent(x[i], g[i], den, step), x0[i], f);
}

__device__ __forceinline__ float apgd_m(float x, float g, float x0, float prev, float den, float eta, float f1) {
  return momentum(x, project(descent(x, g, den, eta), x0, f1), prev);
}

// pass 3 of auto-PGD: z = P(y), m, sum (m - x0)^2
__global__ __launch_bounds__(kThreads) void apgd_l2_sumsq_m(const float* __restrict__ x, const float* __restrict__ g,
                                                            const float* __restrict__ x0, const float* __restrict__ prev,
                                                            int64_t n4, int64_t n, float eps, float eta,
                                                            const double* __restrict__ part_y, int nb,
                                                            double* __restrict__ part_m, float* norms) {
#pragma clang fp contract(off)
  L2_GRID_BEGIN;
  const float den = norms[0] + 1e-10f;
  const float nd = norm_from(part_y, nb);
  if (first == 0) norms[1] = nd;
  const float f1 = ball_factor(eps, nd);
  double acc = 0.0;
  const bma::float4_t* x4 = reinterpret_cast<const bma::float4_t*>(x);
  const bma::float4_t* g4 = reinterpret_cast<const bma::float4_t*>(g);
  const bma::float4_t* o4 = reinterpret_cast<const bma::float4_t*>(x0);
  const bma::float4_t* p4 = reinterpret_cast<const bma::float4_t*>(prev);
  for (int64_t i = first; i < n4; i += stride) {
    const bma::float4_t vx = x4[i], vg = g4[i], v0 = o4[i], vp = p4[i];
    acc += sq(apgd_m(vx.x, vg.x, v0.x, vp.x, den, eta, f1) - v0.x);
    acc += sq(apgd_m(vx.y, vg.y, v0.y, vp.y, den, eta, f1) - v0.y);
    acc += sq(apgd_m(vx.z, vg.z, v0.z, vp.z, den, eta, f1) - v0.z);
    acc += sq(apgd_m(vx.w, vg.w, v0.w, vp.w, den, eta, f1) - v0.w);
  }
  for (int64_t i = n4 * 4 + first; i < n; i += stride)
    acc += sq(apgd_m(x[i], g[i], x0[i], prev[i], den, eta, f1) - x0[i]);
  store_partial(acc, part_m);
}

// pass 4 of auto-PGD: new = P(m); prev, best, out by the two flags, as apgd_step.hip
__global__ __launch_bounds__(kThreads) void apgd_l2_apply(const float* x, const float* __restrict__ g,
                                                          const float* __restrict__ x0, float* __restrict__ prev,
                                                          float* __restrict__ best, float* out, int64_t n4, int64_t n,
                                                          float eps, float eta, int take_best, int restart,
                                                          const double* __restrict__ part_m, int nb, float* norms) {
  L2_GRID_BEGIN;
  const float den = norms[0] + 1e-10f;
  const float f1 = ball_factor(eps, norms[1]);
  const float nm = norm_from(part_m, nb);
  if (first == 0) norms[2] = nm;
  const float f2 = ball_factor(eps, nm);
  const bma::float4_t* x4 = reinterpret_cast<const bma::float4_t*>(x);
  const bma::float4_t* g4 = reinterpret_cast<const bma::float4_t*>(g);
  const bma::float4_t* o4 = reinterpret_cast<const bma::float4_t*>(x0);
  bma::float4_t* p4 = reinterpret_cast<bma::float4_t*>(prev);
  bma::float4_t* b4 = reinterpret_cast<bma::float4_t*>(best);
  bma::float4_t* r4 = reinterpret_cast<bma::float4_t*>(out);
  for (int64_t i = first; i < n4; i += stride) {
    const bma::float4_t vx = x4[i], vg = g4[i], v0 = o4[i], vp = p4[i];
    bma::float4_t r;
    r.x = project(apgd_m(vx.x, vg.x, v0.x, vp.x, den, eta, f1), v0.x, f2);
    r.y = project(apgd_m(vx.y, vg.y, v0.y, vp.y, den, eta, f1), v0.y, f2);
    r.z = project(apgd_m(vx.z, vg.z, v0.z, vp.z, den, eta, f1), v0.z, f2);
    r.w = project(apgd_m(vx.w, vg.w, v0.w, vp.w, den, eta, f1), v0.w, f2);
    if (take_best) b4[i] = r;
    p4[i] = restart ? r : vx;
    r4[i] = r;
  }
  for (int64_t i = n4 * 4 + first; i < n; i += stride) {
    const float vx = x[i], v0 = x0[i];
    const float r = project(apgd_m(vx, g[i], v0, prev[i], den, eta, f1), v0, f2);
    if (take_best) best[i] = r;
    prev[i] = restart ? r : vx;
    out[i] = r;
  }
}

// restart without take_best: out = prev = best, nothing else is read
__global__ __launch_bounds__(kThreads) void apgd_l2_restart(const float* __restrict__ best, float* __restrict__ prev,
                                                            float* out, int64_t n4, int64_t n) {
  L2_GRID_BEGIN;
  const bma::float4_t* b4 = reinterpret_cast<const bma::float4_t*>(best);
  bma::float4_t* p4 = reinterpret_cast<bma::float4_t*>(prev);
  bma::float4_t* r4 = reinterpret_cast<bma::float4_t*>(out);
  for (int64_t i = first; i < n4; i += stride) {
    const bma::float4_t vb = b4[i];
    p4[i] = vb;
    r4[i] = vb;
  }
  for (int64_t i = n4 * 4 + first; i < n; i += stride) {
    const float vb = best[i];
    prev[i] = vb;
    out[i] = vb;
  }
}

struct Shape {
  int64_t n4;   // float4 groups on the vector path (0: a pointer is off the 16-byte grid)
  int blocks;   // workgroups of every pass = partials per norm
};

Shape shape_of(int64_t n, uintptr_t bits) {
  Shape s;
  s.n4 = (bits & 15) == 0 ? n / 4 : 0;
  const int64_t items = s.n4 > 0 ? s.n4 : n;
  int64_t blocks = (items + kThreads - 1) / kThreads;
  s.blocks = static_cast<int>(blocks > kMaxBlocks ? kMaxBlocks : blocks);
  return s;
}

}  // namespace

#define L2_LAUNCH(kernel, bytes_per_px, ...)                                                              \
  do {                                                                                                    \
    BMA_PROF_BEGIN(BMA_K_L2, st, (bytes_per_px) * static_cast<double>(n));                                \
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(sh.blocks)), dim3(kThreads), 0, st, __VA_ARGS__); \
    BMA_PROF_END(BMA_K_L2, st);                                                                           \
    BMA_LAUNCH_CHECK();                                                                                   \
  } while (0)

// three norms' partials, each kMaxBlocks doubles, whatever n is
extern "C" size_t bma_l2_ws_bytes(int64_t n) {
  return n > 0 ? static_cast<size_t>(3 * kMaxBlocks) * sizeof(double) : 0;
}

extern "C" int bma_l2_step(const float* x, const float* g, const float* x0, int64_t n, float eps, float step,
                           float* out, void* ws, float* norms, void* stream) {
  if (n < 0 || (n > 0 && (!x || !g || !x0 || !out || !ws || !norms))) return BMA_EINVAL;
  if (n == 0) return BMA_OK;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g) |
                         reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(out);
  if ((bits & 3) || (reinterpret_cast<uintptr_t>(norms) & 3) || (reinterpret_cast<uintptr_t>(ws) & 7)) return BMA_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Shape sh = shape_of(n, bits);
  double* part_g = static_cast<double*>(ws);
  double* part_y = part_g + kMaxBlocks;
  L2_LAUNCH(l2_sumsq_g, 4.0, g, sh.n4, n, part_g);
  L2_LAUNCH(l2_sumsq_y, 12.0, x, g, x0, sh.n4, n, step, part_g, sh.blocks, part_y, norms);
  L2_LAUNCH(l2_apply, 16.0, x, g, x0, out, sh.n4, n, eps, step, part_y, sh.blocks, norms);
  return BMA_OK;
}

extern "C" int bma_apgd_l2_step(const float* x, const float* g, const float* x0, float* prev, float* best, int64_t n,
                                float eps, float eta, int take_best, int restart, float* out, void* ws, float* norms,
                                void* stream) {
  if (n < 0 || (n > 0 && (!x || !g || !x0 || !prev || !best || !out || !ws || !norms))) return BMA_EINVAL;
  if ((take_best != 0 && take_best != 1) || (restart != 0 && restart != 1)) return BMA_EINVAL;
  if (n > 0 && (prev == best || prev == x || prev == out || best == x || best == out)) return BMA_EINVAL;
  if (n == 0) return BMA_OK;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g) |
                         reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(prev) |
                         reinterpret_cast<uintptr_t>(best) | reinterpret_cast<uintptr_t>(out);
  if ((bits & 3) || (reinterpret_cast<uintptr_t>(norms) & 3) || (reinterpret_cast<uintptr_t>(ws) & 7)) return BMA_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Shape sh = shape_of(n, bits);
  if (restart && !take_best) {
    L2_LAUNCH(apgd_l2_restart, 12.0, best, prev, out, sh.n4, n);
    return BMA_OK;
  }
  double* part_g = static_cast<double*>(ws);
  double* part_y = part_g + kMaxBlocks;
  double* part_m = part_y + kMaxBlocks;
  L2_LAUNCH(l2_sumsq_g, 4.0, g, sh.n4, n, part_g);
  L2_LAUNCH(l2_sumsq_y, 12.0, x, g, x0, sh.n4, n, eta, part_g, sh.blocks, part_y, norms);
  L2_LAUNCH(apgd_l2_sumsq_m, 16.0, x, g, x0, prev, sh.n4, n, eps, eta, part_y, sh.blocks, part_m, norms);
  L2_LAUNCH(apgd_l2_apply, take_best ? 28.0 : 24.0, x, g, x0, prev, best, out, sh.n4, n, eps, eta, take_best, restart,
            part_m, sh.blocks, norms);
  return BMA_OK;
}
