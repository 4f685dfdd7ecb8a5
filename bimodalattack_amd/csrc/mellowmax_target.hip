// a2b -- nanoGCG's mellowmax over the target slice (opt-in, EngineOptions.loss_rule = "mellowmax")
//   the function: reference bimodalattack/utils.py:35-36 (shipped, never called there), applied as nanoGCG applies it:
//   to the NEGATED RAW target logits of a candidate, no softmax over the vocabulary.
//
//   a_j  = alpha * -float(z[j, y_j])                         j = 0..T-1
//   m    = max_j a_j, replaced by 0 when it is +-inf         (torch.logsumexp's rule)
//   s    = sum_j exp(a_j - m)
//   loss = ((log(s) + m) - log(T)) / alpha
//   w_j  = exp(a_j - m) / s                                  d loss / d z[j, y_j] = -w_j
//
// Loss pass: one element per ROW is read (B*T gathers; the V columns are never streamed), so the pass is latency-, not
// bandwidth-bound: a wave per candidate while T fits one sweep of a wave (four candidates per workgroup), a 256-thread
// workgroup per candidate beyond that.  Each lane folds its rows j = lane, lane + n, ... in that order, the lanes are
// merged by an xor butterfly (every lane ends with the same bits) and the four waves in wave order through LDS: the order
// is fixed, two calls on one input are bitwise equal, there are no atomics.  NaN needs no flag: fmaxf skips it, exp keeps
// it, so it reaches s and from there the loss and every weight of the candidate.
//
// dlogits pass: write-only, B*T*V elements (657 MB at B=512, T=20, V=32064, bf16).  One workgroup per row; the row's
// first and last few elements go out one by one where the row does not start or end on a 16-byte boundary (V*elem is
// no multiple of 16, or the caller's block starts off one), everything between as 16-byte vectors of zeros.  The lane
// that owns the label's vector (or head / tail element) puts -w_j * grad_scale into it: one writer per element.

#include "bma_common.h"
#include "bma_profile.h"

namespace {

using bma::uint4_t;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / BMA_WAVE;

template <int DT>
__device__ __forceinline__ float load_elem(const void* base, int64_t i) {
  if (DT == BMA_F32) return static_cast<const float*>(base)[i];
  const uint32_t h = static_cast<const uint16_t*>(base)[i];
  return DT == BMA_BF16 ? bma::bf16_bits_to_f32(h) : bma::f16_bits_to_f32(h);
}

template <int DT>
__device__ __forceinline__ uint32_t elem_bits(float v) {
  if (DT == BMA_F32) return __float_as_uint(v);
  return DT == BMA_BF16 ? bma::f32_to_bf16_bits(v) : bma::f32_to_f16_bits(v);
}

// WG = false: wave `w` of workgroup `g` owns candidate 4*g + w (T <= 64: one sweep).  WG = true: the workgroup owns
// candidate `g` and sweeps its T rows 256 at a time.
template <int DT, bool WG>
__global__ __launch_bounds__(kThreads) void mellowmax_loss_kernel(const void* __restrict__ logits, int64_t ld_cand,
                                                                  int64_t ld_row, const int64_t* __restrict__ labels,
                                                                  int B, int T, int V, float alpha,
                                                                  float* __restrict__ ws, float* __restrict__ loss) {
  const int tid = threadIdx.x;
  const int b = WG ? static_cast<int>(blockIdx.x) : static_cast<int>(blockIdx.x) * kWaves + (tid >> 6);
  if (b >= B) return;                             // (WG: never; else whole waves leave, and nothing below waits on them)
  const int me = WG ? tid : (tid & 63);
  constexpr int n = WG ? kThreads : BMA_WAVE;
  const char* cand = static_cast<const char*>(logits) + static_cast<int64_t>(b) * ld_cand * bma::elem_bytes<DT>::value;

  auto term = [&](int j) -> float {               // alpha * t_j; an out-of-range label poisons the candidate, it is never read
    const int64_t lab = labels[j];
    if (lab < 0 || lab >= V) return NAN;
    return alpha * -load_elem<DT>(cand, static_cast<int64_t>(j) * ld_row + lab);
  };
  __shared__ float sm[2][kWaves];
  auto across_waves = [&](float v, int slot, bool is_max) -> float {
    if (!WG) return v;
    if ((tid & 63) == 0) sm[slot][tid >> 6] = v;
    __syncthreads();
    float r = sm[slot][0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) r = is_max ? fmaxf(r, sm[slot][w]) : r + sm[slot][w];
    return r;
  };

  // the first sweep's term stays in a register; later sweeps (WG only) gather theirs again
  const float a0 = me < T ? term(me) : -INFINITY;
  float m = a0;
  for (int j = me + n; j < T; j += n) m = fmaxf(m, term(j));
  m = across_waves(bma::wave_max(m), 0, true);
  if (fabsf(m) == INFINITY) m = 0.0f;             // an all-NaN candidate arrives here as -inf, too
  float s = me < T ? expf(a0 - m) : 0.0f;
  for (int j = me + n; j < T; j += n) s += expf(term(j) - m);
  s = across_waves(bma::wave_sum(s), 1, false);

  float* w = ws + static_cast<int64_t>(b) * T;
  if (me < T) w[me] = expf(a0 - m) / s;
  for (int j = me + n; j < T; j += n) w[j] = expf(term(j) - m) / s;
  if (me == 0) loss[b] = ((logf(s) + m) - logf(static_cast<float>(T))) / alpha;
}

template <int DT>
__global__ __launch_bounds__(kThreads) void mellowmax_dlogits_kernel(const int64_t* __restrict__ labels, int T, int V,
                                                                     const float* __restrict__ ws,
                                                                     void* __restrict__ dlogits, float grad_scale) {
  constexpr int ES = bma::elem_bytes<DT>::value, NE = 16 / ES;
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t lab64 = labels[row % T];
  const int lab = (lab64 >= 0 && lab64 < V) ? static_cast<int>(lab64) : -1;      // out of range: the row is all zeros
  const uint32_t bits = elem_bits<DT>(-ws[row] * grad_scale);
  char* obase = static_cast<char*>(dlogits) + row * V * ES;
  auto put = [&](int i) {                          // one element, by the lane that owns it
    const uint32_t v = i == lab ? bits : 0u;
    if (DT == BMA_F32) reinterpret_cast<uint32_t*>(obase)[i] = v;
    else reinterpret_cast<uint16_t*>(obase)[i] = static_cast<uint16_t>(v);
  };
  // [0, head) up to the first 16-byte boundary, [head, tail) as nvec vectors, [tail, V) the rest
  const int misfit = static_cast<int>(reinterpret_cast<uintptr_t>(obase) & 15);
  const int head = min(V, ((16 - misfit) & 15) / ES);
  const int nvec = (V - head) / NE;
  const int tail = head + nvec * NE;
  if (tid < head) put(tid);
  if (tid < V - tail) put(tail + tid);
  uint4_t* q = reinterpret_cast<uint4_t*>(obase + head * ES);
  const int lv = (lab >= head && lab < tail) ? (lab - head) / NE : -1;
  for (int i = tid; i < nvec; i += kThreads) {
    uint32_t word[4] = {0u, 0u, 0u, 0u};
    if (i == lv) {
      const int k = (lab - head) % NE;
      if (DT == BMA_F32) word[k] = bits;
      else word[k >> 1] = bits << (16 * (k & 1));
    }
    uint4_t v;
    v.x = word[0]; v.y = word[1]; v.z = word[2]; v.w = word[3];
    q[i] = v;
  }
}

template <int DT>
int launch(const void* logits, int64_t ld_cand, int64_t ld_row, const int64_t* labels, int B, int T, int V, float alpha,
           float* ws, float* loss, void* dlogits, float grad_scale, hipStream_t st) {
  constexpr int ES = bma::elem_bytes<DT>::value;
  const int64_t BT = static_cast<int64_t>(B) * T;
  BMA_PROF_BEGIN(BMA_K_MELLOWMAX, st, static_cast<double>(BT) * (ES + 8 + 4) + 4.0 * B);
  if (T <= BMA_WAVE)
    hipLaunchKernelGGL((mellowmax_loss_kernel<DT, false>), dim3((B + kWaves - 1) / kWaves), dim3(kThreads), 0, st, logits,
                       ld_cand, ld_row, labels, B, T, V, alpha, ws, loss);
  else
    hipLaunchKernelGGL((mellowmax_loss_kernel<DT, true>), dim3(B), dim3(kThreads), 0, st, logits, ld_cand, ld_row, labels,
                       B, T, V, alpha, ws, loss);
  BMA_PROF_END(BMA_K_MELLOWMAX, st);
  BMA_LAUNCH_CHECK();
  if (dlogits) {
    BMA_PROF_BEGIN(BMA_K_MELLOWMAX_DLOGITS, st, static_cast<double>(BT) * V * ES);
    hipLaunchKernelGGL((mellowmax_dlogits_kernel<DT>), dim3(static_cast<unsigned>(BT)), dim3(kThreads), 0, st, labels, T, V,
                       ws, dlogits, grad_scale);
    BMA_PROF_END(BMA_K_MELLOWMAX_DLOGITS, st);
    BMA_LAUNCH_CHECK();
  }
  return BMA_OK;
}

}  // namespace

extern "C" size_t bma_mellowmax_target_ws_bytes(int B, int T) {
  if (B < 0 || T < 0) return 0;
  return static_cast<size_t>(B) * static_cast<size_t>(T) * 4;
}

extern "C" int bma_mellowmax_target(const void* logits, int64_t ld_cand, int64_t ld_row, const int64_t* labels, int B,
                                    int T, int V, int dtype, float alpha, float* ws, float* loss, void* dlogits,
                                    float grad_scale, void* stream) {
  if (B < 0 || T < 1 || V < 1 || ld_row < V || ld_cand < 0) return BMA_EINVAL;
  if (!(alpha > 0.0f) || alpha == INFINITY) return BMA_EINVAL;        // NaN fails the first test
  if (dtype != BMA_F32 && dtype != BMA_BF16 && dtype != BMA_F16) return BMA_EDTYPE;
  if (B == 0) return BMA_OK;
  if (!logits || !labels || !ws || !loss) return BMA_EINVAL;
  if (static_cast<int64_t>(B) * T > 0x7fffffffLL) return BMA_ELIMIT;
  const uintptr_t es = dtype == BMA_F32 ? 4 : 2;
  if (reinterpret_cast<uintptr_t>(logits) % es || reinterpret_cast<uintptr_t>(dlogits) % es ||
      reinterpret_cast<uintptr_t>(ws) % 4 || reinterpret_cast<uintptr_t>(loss) % 4 ||
      reinterpret_cast<uintptr_t>(labels) % 8)
    return BMA_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case BMA_F32: return launch<BMA_F32>(logits, ld_cand, ld_row, labels, B, T, V, alpha, ws, loss, dlogits, grad_scale, st);
    case BMA_BF16: return launch<BMA_BF16>(logits, ld_cand, ld_row, labels, B, T, V, alpha, ws, loss, dlogits, grad_scale, st);
    default: return launch<BMA_F16>(logits, ld_cand, ld_row, labels, B, T, V, alpha, ws, loss, dlogits, grad_scale, st);
  }
}
