// a5 / a5b / a5c -- the PGD image update: two rules (plain, auto-PGD), each in two threat models
// (the L-inf box, the L2 ball).  One file: the per-pixel expressions, the write-back and the loops
// are written once and the four entry points of include/bma.h are built from them.
//
// a5 -- PGD L-inf step (reference bimodal_attack.py:1030-1037), bma_linf_step:
//
//   out = clamp(clamp(x - step*sign(g), x0-eps, x0+eps), 0, 1)      fp32, exact
//
// a5b -- auto-PGD L-inf step (reference bimodal_attack.py:1039-1110, perform_autopgd_step),
// bma_apgd_step.  The per-pixel part of one call; the host (pgd.ApgdState) keeps eta, the losses
// and the counters and passes the two decisions of the call as flags:
//
//   z    = clamp(max(min(x - eta*sign(g), x0+eps), x0-eps), 0, 1)
//   new  = clamp(max(min((x + 0.75*(z-x)) + 0.25*(x-prev), x0+eps), x0-eps), 0, 1)
//   prev = x
//   take_best:  best = new                    (the step loss improved on the best one)
//   restart:    out = prev = best             (a checkpoint halved eta)
//   otherwise:  out = new
//
// With restart and no take_best the kernel reads best only (x, g, x0, prev are not touched).
//
// a5c -- both rules in the L2 ball (opt-in, EngineOptions.pgd_norm = "l2"; the reference has no L2
// update), bma_l2_step / bma_apgd_l2_step.  The arithmetic contract is in include/bma.h next to
// the entry points:
//
//   nrm(v) = float( sqrt( sum_i double(v_i)^2 ) )            fp64 accumulation, rounded once
//   P(y)   = clamp01( x0 + (y - x0) * min(eps / nrm(y - x0), 1) )
//   u      = g / (nrm(g) + 1e-10f)
//   plain:     out = P(x - step*u)
//   auto-PGD:  z = P(x - eta*u);  m = (x + 0.75*(z - x)) + 0.25*(x - prev);  new = P(m)
//              prev / best / take_best / restart as bma_apgd_step
//
// The box rules stream (linf_step_*, apgd_step_*).  HBM-bound, no reductions: a5 moves 16
// algorithmic bytes per pixel (3 reads + 1 write), a5b 16 B read (x, g, x0, prev) + 8 B written
// (out, prev), + 4 B when best is written.  At the LLaVA image size (338,688 px, 5.4 MB) the launch
// is latency-bound; at the Gemma size (2,408,448 px, 38.5 MB) it streams.  One float4 per lane per
// access (16 B/lane, 1 KiB per wave-instruction), grid-stride over <= 2048 workgroups of 256 lanes
// when every pointer is 16-byte aligned, and a scalar kernel of the same shape for the last n % 4
// pixels (or for all of them when a pointer is not).
//
// The ball rules are not one streaming launch: every norm is a reduction over the whole image that
// the next expression depends on.  The call is a chain of ordinary launches on the caller's stream
// (no cooperative grid, no flag anybody waits on):
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
// per CU, 16 waves each) rather than the streaming 2048 x 256: 256 dependent fp64 adds instead of
// 2048.  The vector / tail split is the streaming one, but both loops run in the same launch, so a
// workgroup's partial covers both.
//
// Bit-exactness notes, the contract of this file:
//  * sign() is torch's ((g>0) - (g<0): 0 for NaN and -0.0); step*sign and eta*sign are exact, so in
//    linf_one contracting the product into an FMA cannot change the result (it carries no pragma).
//  * linf_one's two clamps and clamp01 are compare+select: NaN and -0.0 propagate exactly as
//    torch.clamp propagates them.  torch.min / torch.max (auto-PGD's box) propagate a NaN from
//    either operand and return the FIRST operand on a tie (+-0), unlike compare+select.
//  * Everywhere else FMA contraction is off: the momentum line and the ball's expressions are
//    rounded op by op in fp32 as the reference / the torch restatement evaluates them.
//  * fp32 division is the IEEE-rounded one (the build has no fast-math); min(eps/nrm, 1) propagates
//    NaN like torch.minimum.

#include "bma_common.h"
#include "bma_profile.h"

namespace {

using bma::float4_t;

// ------------------------------------------------------------------ per-pixel expressions
__device__ __forceinline__ float clamp01(float y) {
  y = y < 0.0f ? 0.0f : y;
  return y > 1.0f ? 1.0f : y;
}

__device__ __forceinline__ float torch_sign(float g) { return (g > 0.0f ? 1.0f : 0.0f) - (g < 0.0f ? 1.0f : 0.0f); }

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

__device__ __forceinline__ float linf_one(float x, float g, float x0, float eps, float step) {
  float y = x - step * torch_sign(g);
  const float lo = x0 - eps, hi = x0 + eps;
  y = y < lo ? lo : y;
  y = y > hi ? hi : y;
  return clamp01(y);
}

__device__ __forceinline__ float momentum(float x, float z, float prev) {
#pragma clang fp contract(off)
  const float a = 0.75f * (z - x);
  const float b = 0.25f * (x - prev);
  return (x + a) + b;
}

__device__ __forceinline__ float apgd_one(float x, float g, float x0, float prev, float eps, float eta) {
#pragma clang fp contract(off)
  const float hi = x0 + eps, lo = x0 - eps;
  const float z = clamp01(torch_max(torch_min(x - eta * torch_sign(g), hi), lo));
  return clamp01(torch_max(torch_min(momentum(x, z, prev), hi), lo));
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

__device__ __forceinline__ float apgd_m(float x, float g, float x0, float prev, float den, float eta, float f1) {
  return momentum(x, project(descent(x, g, den, eta), x0, f1), prev);
}

// f on one pixel, or on each of the four of a float4
template <class F, class... A>
__device__ __forceinline__ float each(F f, float a0, A... a) { return f(a0, a...); }

template <class F, class... A>
__device__ __forceinline__ float4_t each(F f, float4_t a0, A... a) {
  float4_t r;
  r.x = f(a0.x, a.x...);
  r.y = f(a0.y, a.y...);
  r.z = f(a0.z, a.z...);
  r.w = f(a0.w, a.w...);
  return r;
}

// acc += double(v)^2, a float4's pixels in x, y, z, w order.  The square of a widened fp32 value is exact in fp64, so
// whether the compiler fuses it into the add cannot change a bit.
__device__ __forceinline__ void add_sq(double& acc, float v) {
  const double d = static_cast<double>(v);
  acc += d * d;
}

__device__ __forceinline__ void add_sq(double& acc, float4_t v) {
  add_sq(acc, v.x);
  add_sq(acc, v.y);
  add_sq(acc, v.z);
  add_sq(acc, v.w);
}

// ------------------------------------------------------------------ loops, auto-PGD write-back (T: float4_t or float)
struct Grid {
  int64_t first, stride;   // this lane's index in the grid, the grid's lanes
};

// Expanded in the __global__ function itself: only there does the compiler know that every workgroup has blockDim.x
// lanes and read it with one scalar load (in a __device__ helper it selects between the size and a remainder).
#define THIS_GRID \
  Grid { static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x, static_cast<int64_t>(gridDim.x) * blockDim.x }

template <class Body>
__device__ __forceinline__ void grid_stride(Grid grid, int64_t begin, int64_t end, Body body) {
  for (int64_t i = begin + grid.first; i < end; i += grid.stride) body(i);
}

// the new image r of an auto-PGD call into the state and the output (vx: the call's input image)
template <class T>
__device__ __forceinline__ void write_back(T r, T vx, int64_t i, T* prev, T* best, T* out, int take_best, int restart) {
  if (take_best) best[i] = r;
  prev[i] = restart ? r : vx;
  out[i] = r;
}

// restart without take_best: out = prev = best, nothing else is read
template <class T>
__device__ __forceinline__ void restart_from_best(int64_t i, const T* best, T* prev, T* out) {
  const T vb = best[i];
  prev[i] = vb;
  out[i] = vb;
}

// ------------------------------------------------------------------ the box: streaming kernels
constexpr int kStreamThreads = 256;
constexpr int kStreamMaxBlocks = 2048;

template <class T>
__device__ __forceinline__ void linf_loop(Grid grid, const T* x, const T* g, const T* x0, T* out, int64_t begin,
                                          int64_t end, float eps, float step) {
  grid_stride(grid, begin, end, [=](int64_t i) {
    out[i] = each([=](float x, float g, float x0) { return linf_one(x, g, x0, eps, step); }, x[i], g[i], x0[i]);
  });
}

template <class T>
__device__ __forceinline__ void apgd_loop(Grid grid, const T* x, const T* g, const T* x0, T* prev, T* best, T* out,
                                          int64_t begin, int64_t end, float eps, float eta, int take_best, int restart) {
  grid_stride(grid, begin, end, [=](int64_t i) {
    if (restart && !take_best) {
      restart_from_best(i, best, prev, out);
      return;
    }
    const T vx = x[i];
    const T r = each([=](float x, float g, float x0, float prev) { return apgd_one(x, g, x0, prev, eps, eta); }, vx, g[i],
                     x0[i], prev[i]);
    write_back(r, vx, i, prev, best, out, take_best, restart);
  });
}

__global__ __launch_bounds__(kStreamThreads) void linf_step_vec4(const float4_t* x, const float4_t* __restrict__ g,
                                                                 const float4_t* __restrict__ x0, float4_t* out, int64_t n4,
                                                                 float eps, float step) {
  linf_loop(THIS_GRID, x, g, x0, out, 0, n4, eps, step);
}

__global__ __launch_bounds__(kStreamThreads) void linf_step_scalar(const float* x, const float* g, const float* x0,
                                                                   float* out, int64_t begin, int64_t n, float eps,
                                                                   float step) {
  linf_loop(THIS_GRID, x, g, x0, out, begin, n, eps, step);
}

__global__ __launch_bounds__(kStreamThreads) void apgd_step_vec4(const float4_t* x, const float4_t* __restrict__ g,
                                                                 const float4_t* __restrict__ x0, float4_t* __restrict__ prev,
                                                                 float4_t* __restrict__ best, float4_t* out, int64_t n4,
                                                                 float eps, float eta, int take_best, int restart) {
  apgd_loop(THIS_GRID, x, g, x0, prev, best, out, 0, n4, eps, eta, take_best, restart);
}

__global__ __launch_bounds__(kStreamThreads) void apgd_step_scalar(const float* x, const float* g, const float* x0,
                                                                   float* prev, float* best, float* out, int64_t begin,
                                                                   int64_t n, float eps, float eta, int take_best,
                                                                   int restart) {
  apgd_loop(THIS_GRID, x, g, x0, prev, best, out, begin, n, eps, eta, take_best, restart);
}

// ------------------------------------------------------------------ the ball: the reduction chain
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / BMA_WAVE;
constexpr int kMaxBlocks = 256;

// float4 groups [0, n4), then the pixels behind them [4*n4, n), in one launch: body(i, T()) says which
template <class Body>
__device__ __forceinline__ void vec_then_tail(Grid grid, int64_t n4, int64_t n, Body body) {
  grid_stride(grid, 0, n4, [&](int64_t i) { body(i, float4_t()); });
  grid_stride(grid, n4 * 4, n, [&](int64_t i) { body(i, float()); });
}

template <class T>
__device__ __forceinline__ const T* as(const float* p, T) { return reinterpret_cast<const T*>(p); }

template <class T>
__device__ __forceinline__ T* as(float* p, T) { return reinterpret_cast<T*>(p); }

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

__global__ __launch_bounds__(kThreads) void l2_sumsq_g(const float* __restrict__ g, int64_t n4, int64_t n,
                                                       double* __restrict__ part) {
  const Grid grid = THIS_GRID;
  double acc = 0.0;
  vec_then_tail(grid, n4, n, [&](int64_t i, auto t) { add_sq(acc, as(g, t)[i]); });
  store_partial(acc, part);
}

// pass 2 of both rules: y = x - step*u, sum (y - x0)^2
__global__ __launch_bounds__(kThreads) void l2_sumsq_y(const float* __restrict__ x, const float* __restrict__ g,
                                                       const float* __restrict__ x0, int64_t n4, int64_t n, float step,
                                                       const double* __restrict__ part_g, int nb,
                                                       double* __restrict__ part_y, float* __restrict__ norms) {
#pragma clang fp contract(off)
  const Grid grid = THIS_GRID;
  const float ng = norm_from(part_g, nb);
  if (grid.first == 0) norms[0] = ng;
  const float den = ng + 1e-10f;
  double acc = 0.0;
  vec_then_tail(grid, n4, n, [&](int64_t i, auto t) {
    add_sq(acc, each([=](float x, float g, float x0) { return descent(x, g, den, step) - x0; }, as(x, t)[i], as(g, t)[i],
                     as(x0, t)[i]));
  });
  store_partial(acc, part_y);
}

// pass 3 of the plain step: out = P(y).  out may alias x (each lane reads its pixel before it writes it).
__global__ __launch_bounds__(kThreads) void l2_apply(const float* x, const float* __restrict__ g,
                                                     const float* __restrict__ x0, float* out, int64_t n4, int64_t n,
                                                     float eps, float step, const double* __restrict__ part_y, int nb,
                                                     float* norms) {
  const Grid grid = THIS_GRID;
  const float den = norms[0] + 1e-10f;
  const float nd = norm_from(part_y, nb);
  if (grid.first == 0) norms[1] = nd;
  const float f = ball_factor(eps, nd);
  vec_then_tail(grid, n4, n, [&](int64_t i, auto t) {
    as(out, t)[i] = each([=](float x, float g, float x0) { return project(descent(x, g, den, step), x0, f); }, as(x, t)[i],
                         as(g, t)[i], as(x0, t)[i]);
  });
}

// pass 3 of auto-PGD: z = P(y), m, sum (m - x0)^2
__global__ __launch_bounds__(kThreads) void apgd_l2_sumsq_m(const float* __restrict__ x, const float* __restrict__ g,
                                                            const float* __restrict__ x0, const float* __restrict__ prev,
                                                            int64_t n4, int64_t n, float eps, float eta,
                                                            const double* __restrict__ part_y, int nb,
                                                            double* __restrict__ part_m, float* norms) {
#pragma clang fp contract(off)
  const Grid grid = THIS_GRID;
  const float den = norms[0] + 1e-10f;
  const float nd = norm_from(part_y, nb);
  if (grid.first == 0) norms[1] = nd;
  const float f1 = ball_factor(eps, nd);
  double acc = 0.0;
  vec_then_tail(grid, n4, n, [&](int64_t i, auto t) {
    add_sq(acc, each([=](float x, float g, float x0, float prev) { return apgd_m(x, g, x0, prev, den, eta, f1) - x0; },
                     as(x, t)[i], as(g, t)[i], as(x0, t)[i], as(prev, t)[i]));
  });
  store_partial(acc, part_m);
}

// pass 4 of auto-PGD: new = P(m); prev, best, out by the two flags
__global__ __launch_bounds__(kThreads) void apgd_l2_apply(const float* x, const float* __restrict__ g,
                                                          const float* __restrict__ x0, float* __restrict__ prev,
                                                          float* __restrict__ best, float* out, int64_t n4, int64_t n,
                                                          float eps, float eta, int take_best, int restart,
                                                          const double* __restrict__ part_m, int nb, float* norms) {
  const Grid grid = THIS_GRID;
  const float den = norms[0] + 1e-10f;
  const float f1 = ball_factor(eps, norms[1]);
  const float nm = norm_from(part_m, nb);
  if (grid.first == 0) norms[2] = nm;
  const float f2 = ball_factor(eps, nm);
  vec_then_tail(grid, n4, n, [&](int64_t i, auto t) {
    const auto vx = as(x, t)[i];
    const auto r = each([=](float x, float g, float x0, float prev) {
      return project(apgd_m(x, g, x0, prev, den, eta, f1), x0, f2);
    }, vx, as(g, t)[i], as(x0, t)[i], as(prev, t)[i]);
    write_back(r, vx, i, as(prev, t), as(best, t), as(out, t), take_best, restart);
  });
}

__global__ __launch_bounds__(kThreads) void apgd_l2_restart(const float* __restrict__ best, float* __restrict__ prev,
                                                            float* out, int64_t n4, int64_t n) {
  const Grid grid = THIS_GRID;
  vec_then_tail(grid, n4, n, [&](int64_t i, auto t) { restart_from_best(i, as(best, t), as(prev, t), as(out, t)); });
}

// ------------------------------------------------------------------ host side
template <class... P>
bool any_null(P... p) {
  return (... || (p == nullptr));
}

// every image pointer OR'ed: bits & 3 is BMA_EALIGN, bits & 15 decides float4 or scalar
template <class... P>
uintptr_t address_bits(P... p) {
  return (... | reinterpret_cast<uintptr_t>(p));
}

int block_count(int64_t items, int threads, int max_blocks) {
  const int64_t blocks = (items + threads - 1) / threads;
  return static_cast<int>(blocks > max_blocks ? max_blocks : blocks);
}

// auto-PGD: a flag is 0 or 1; prev and best are state buffers of their own (only out may alias x)
bool apgd_args_ok(const float* x, const float* prev, const float* best, const float* out, int64_t n, int take_best,
                  int restart) {
  if ((take_best != 0 && take_best != 1) || (restart != 0 && restart != 1)) return false;
  return !(n > 0 && (prev == best || prev == x || prev == out || best == x || best == out));
}

const float4_t* v4(const float* p) { return reinterpret_cast<const float4_t*>(p); }
float4_t* v4(float* p) { return reinterpret_cast<float4_t*>(p); }

// The streaming launch pair: vec4(grid, n4) over the float4 groups when every pointer is 16-byte aligned, then
// scalar(grid, done) over what is left.  Only the float4 launch is profiled, px_bytes algorithmic bytes per pixel.
template <class Vec4, class Scalar>
int stream_launch(int kernel_id, double px_bytes, int64_t n, uintptr_t bits, hipStream_t st, Vec4 vec4, Scalar scalar) {
  int64_t done = 0;
  if ((bits & 15) == 0 && n >= 4) {
    const int64_t n4 = n / 4;
    BMA_PROF_BEGIN(kernel_id, st, px_bytes * static_cast<double>(n4) * 4.0);
    vec4(dim3(block_count(n4, kStreamThreads, kStreamMaxBlocks)), n4);
    BMA_PROF_END(kernel_id, st);
    BMA_LAUNCH_CHECK();
    done = n4 * 4;
  }
  if (done < n) {
    scalar(dim3(block_count(n - done, kStreamThreads, kStreamMaxBlocks)), done);
    BMA_LAUNCH_CHECK();
  }
  return BMA_OK;
}

struct Shape {
  int64_t n4;        // float4 groups on the vector path (0: a pointer is off the 16-byte grid)
  int blocks;        // workgroups of every pass = partials per norm
};

Shape shape_of(int64_t n, uintptr_t bits) {
  Shape s;
  s.n4 = (bits & 15) == 0 ? n / 4 : 0;
  s.blocks = block_count(s.n4 > 0 ? s.n4 : n, kThreads, kMaxBlocks);
  return s;
}

bool l2_scratch_misaligned(const void* ws, const float* norms) {
  return (reinterpret_cast<uintptr_t>(norms) & 3) || (reinterpret_cast<uintptr_t>(ws) & 7);
}

}  // namespace

#define L2_LAUNCH(kernel, bytes_per_px, ...)                                                \
  do {                                                                                      \
    BMA_PROF_BEGIN(BMA_K_L2, st, (bytes_per_px) * static_cast<double>(n));                  \
    hipLaunchKernelGGL(kernel, dim3(sh.blocks), dim3(kThreads), 0, st, __VA_ARGS__);        \
    BMA_PROF_END(BMA_K_L2, st);                                                             \
    BMA_LAUNCH_CHECK();                                                                     \
  } while (0)

extern "C" int bma_linf_step(const float* x, const float* g, const float* x0, int64_t n, float eps, float step,
                             float* out, void* stream) {
  if (n < 0 || (n > 0 && any_null(x, g, x0, out))) return BMA_EINVAL;
  if (n == 0) return BMA_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uintptr_t bits = address_bits(x, g, x0, out);
  if (bits & 3) return BMA_EALIGN;
  return stream_launch(
      BMA_K_LINF, 16.0, n, bits, st,
      [&](dim3 grid, int64_t n4) {
        hipLaunchKernelGGL(linf_step_vec4, grid, dim3(kStreamThreads), 0, st, v4(x), v4(g), v4(x0), v4(out), n4, eps, step);
      },
      [&](dim3 grid, int64_t done) {
        hipLaunchKernelGGL(linf_step_scalar, grid, dim3(kStreamThreads), 0, st, x, g, x0, out, done, n, eps, step);
      });
}

extern "C" int bma_apgd_step(const float* x, const float* g, const float* x0, float* prev, float* best, int64_t n,
                             float eps, float eta, int take_best, int restart, float* out, void* stream) {
  if (n < 0 || (n > 0 && any_null(x, g, x0, prev, best, out))) return BMA_EINVAL;
  if (!apgd_args_ok(x, prev, best, out, n, take_best, restart)) return BMA_EINVAL;
  if (n == 0) return BMA_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uintptr_t bits = address_bits(x, g, x0, prev, best, out);
  if (bits & 3) return BMA_EALIGN;
  const double px_bytes = (restart && !take_best) ? 12.0 : (take_best ? 28.0 : 24.0);
  return stream_launch(
      BMA_K_APGD, px_bytes, n, bits, st,
      [&](dim3 grid, int64_t n4) {
        hipLaunchKernelGGL(apgd_step_vec4, grid, dim3(kStreamThreads), 0, st, v4(x), v4(g), v4(x0), v4(prev), v4(best),
                           v4(out), n4, eps, eta, take_best, restart);
      },
      [&](dim3 grid, int64_t done) {
        hipLaunchKernelGGL(apgd_step_scalar, grid, dim3(kStreamThreads), 0, st, x, g, x0, prev, best, out, done, n, eps,
                           eta, take_best, restart);
      });
}

// three norms' partials, each kMaxBlocks doubles, whatever n is
extern "C" size_t bma_l2_ws_bytes(int64_t n) {
  return n > 0 ? static_cast<size_t>(3 * kMaxBlocks) * sizeof(double) : 0;
}

extern "C" int bma_l2_step(const float* x, const float* g, const float* x0, int64_t n, float eps, float step,
                           float* out, void* ws, float* norms, void* stream) {
  if (n < 0 || (n > 0 && any_null(x, g, x0, out, ws, norms))) return BMA_EINVAL;
  if (n == 0) return BMA_OK;
  const uintptr_t bits = address_bits(x, g, x0, out);
  if ((bits & 3) || l2_scratch_misaligned(ws, norms)) return BMA_EALIGN;
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
  if (n < 0 || (n > 0 && any_null(x, g, x0, prev, best, out, ws, norms))) return BMA_EINVAL;
  if (!apgd_args_ok(x, prev, best, out, n, take_best, restart)) return BMA_EINVAL;
  if (n == 0) return BMA_OK;
  const uintptr_t bits = address_bits(x, g, x0, prev, best, out);
  if ((bits & 3) || l2_scratch_misaligned(ws, norms)) return BMA_EALIGN;
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
