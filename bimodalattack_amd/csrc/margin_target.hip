// a2c -- the Carlini-Wagner margin over the target slice (opt-in, EngineOptions.loss_rule = "margin")
//   per candidate b and target row j with label y_j, z = float(logits[b, j, :]):
//
//   o_j  = max over v != y_j of z_v,  i_j = the FIRST index v != y_j with z_v == o_j   (o_j = z[i_j])
//   m_j  = o_j - z[y_j]
//   loss = (sum_j max(m_j, -kappa)) / T                     summed in row order
//   a_j  = m_j >= -kappa                                    dlogits: -a_j*g at y_j, +a_j*g at i_j, g = grad_scale / T
//   match = every row's first argmax over ALL v is its label (bma_ce_target's early-stop test)
//
// Row pass: HBM-bound like ce_rows_kernel -- the B*T rows of V logits are read exactly once, one 256-thread workgroup
// per row, 16-byte vectors with four loads in flight per lane; a row that does not start or end on the 16-byte grid
// (small or odd V, ld_row > V, a block that starts off the grid) gives its first and last few elements to single
// lanes.  A lane keeps ONE (value, first index) pair, over v != y: the label's element is taken out of the maximum as
// it goes by.  The argmax over all v that the early-stop test needs follows from that pair and z[y_j], which the
// margin reads anyway: it is y_j exactly when z[y_j] > o_j, or z[y_j] == o_j with y_j < i_j.  Ties go to the lower
// index at every level: inside a vector, between a lane's vectors (which do not arrive in index order), in the xor
// butterfly across the wave and between the four waves through LDS.  fmaxf skips NaN, so a NaN flag rides along; it
// is taken before the label is taken out, so a NaN at the label counts.  Maxima start from -INFINITY: a row of -inf
// keeps its first index.
//
// A second tiny launch folds the T row terms of a candidate in row order (two calls bitwise equal, no atomics) and
// ANDs the row hits.  dlogits pass: write-only, one workgroup per row, element-wise head and tail around 16-byte
// vectors as mellowmax_dlogits_kernel, with two non-zero elements per active row; they may share a vector, or sit
// one in the head and one in the tail.  Every element is written by exactly one lane.
//
// Scratch layout (`ws`, 3*B*T 4-byte words): [0,BT) m f32 | [BT,2BT) i int32 (-1: none) | [2BT,3BT) row hit int32.

#include "bma_common.h"
#include "bma_profile.h"

namespace {

using bma::uint4_t;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / BMA_WAVE;
constexpr int kNone = 0x7fffffff;

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

template <int DT>
__device__ __forceinline__ void unpack(const uint4_t& w, float* f) {
  if (DT == BMA_F32) {
    f[0] = __uint_as_float(w.x); f[1] = __uint_as_float(w.y);
    f[2] = __uint_as_float(w.z); f[3] = __uint_as_float(w.w);
  } else {
    f[0] = bma::unpack16<DT>(w.x, 0); f[1] = bma::unpack16<DT>(w.x, 1);
    f[2] = bma::unpack16<DT>(w.y, 0); f[3] = bma::unpack16<DT>(w.y, 1);
    f[4] = bma::unpack16<DT>(w.z, 0); f[5] = bma::unpack16<DT>(w.z, 1);
    f[6] = bma::unpack16<DT>(w.w, 0); f[7] = bma::unpack16<DT>(w.w, 1);
  }
}

struct Best {
  float v;    // the best value over v != y so far (NaN skipped)
  int i;      // its first index; kNone: nothing seen yet
  bool bad;   // a NaN went by (the label's element included)
};

__device__ __forceinline__ void best_merge(Best& a, float v, int i) {
  if (v > a.v || (v == a.v && i < a.i)) { a.v = v; a.i = i; }
}

// N consecutive elements starting at index `first`; `lab` (-1: no label to take out) is excluded from the maximum.
template <int N>
__device__ __forceinline__ void best_push(Best& r, float* f, int first, int lab) {
  bool nan = false;
#pragma unroll
  for (int j = 0; j < N; ++j) nan |= f[j] != f[j];
  r.bad |= nan;
  const unsigned k = static_cast<unsigned>(lab - first);
  if (k < static_cast<unsigned>(N)) {             // the label's own chunk: one lane of the row, once
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (j == static_cast<int>(k)) f[j] = NAN;   // skipped by fmaxf, equal to nothing
  }
  float cm = f[0];
#pragma unroll
  for (int j = 1; j < N; ++j) cm = fmaxf(cm, f[j]);
  if (cm > r.v || (cm == r.v && first < r.i)) {   // this lane's chunks are not monotone in index
#pragma unroll
    for (int j = N - 1; j >= 0; --j)
      if (f[j] == cm) { r.i = first + j; r.v = f[j]; }
  }
}

// One workgroup per row: [0, head) up to the first 16-byte boundary, [head, tail) as nvec vectors, [tail, V) the rest.
template <int DT>
__global__ __launch_bounds__(kThreads) void margin_rows_kernel(const void* __restrict__ logits, int64_t ld_cand,
                                                               int64_t ld_row, const int64_t* __restrict__ labels,
                                                               int T, int V, float* __restrict__ ws, int64_t BT) {
  constexpr int ES = bma::elem_bytes<DT>::value, NE = 16 / ES;
  const int64_t row = blockIdx.x;
  const int b = static_cast<int>(row / T), t = static_cast<int>(row % T);
  const int64_t off = static_cast<int64_t>(b) * ld_cand + static_cast<int64_t>(t) * ld_row;
  const char* base = static_cast<const char*>(logits) + off * ES;
  const int tid = threadIdx.x;
  const int64_t lab64 = labels[t];
  const int lab = (lab64 >= 0 && lab64 < V) ? static_cast<int>(lab64) : -1;   // out of range: never read through

  const int misfit = static_cast<int>(reinterpret_cast<uintptr_t>(base) & 15);
  const int head = min(V, ((16 - misfit) & 15) / ES);
  const int nvec = (V - head) / NE;
  const int tail = head + nvec * NE;

  Best st;
  st.v = -INFINITY; st.i = kNone; st.bad = false;
  if (tid < head) {
    float f[1] = {load_elem<DT>(base, tid)};
    best_push<1>(st, f, tid, lab);
  }
  if (tid < V - tail) {
    float f[1] = {load_elem<DT>(base, tail + tid)};
    best_push<1>(st, f, tail + tid, lab);
  }
  const uint4_t* p = reinterpret_cast<const uint4_t*>(base + head * ES);
  int i = tid;
  // four 16-byte loads in flight per lane (4 KiB per wave per trip)
  for (; i + 3 * kThreads < nvec; i += 4 * kThreads) {
    const uint4_t w0 = p[i], w1 = p[i + kThreads], w2 = p[i + 2 * kThreads], w3 = p[i + 3 * kThreads];
    float f[NE];
    unpack<DT>(w0, f); best_push<NE>(st, f, head + i * NE, lab);
    unpack<DT>(w1, f); best_push<NE>(st, f, head + (i + kThreads) * NE, lab);
    unpack<DT>(w2, f); best_push<NE>(st, f, head + (i + 2 * kThreads) * NE, lab);
    unpack<DT>(w3, f); best_push<NE>(st, f, head + (i + 3 * kThreads) * NE, lab);
  }
  for (; i < nvec; i += kThreads) {
    float f[NE];
    unpack<DT>(p[i], f);
    best_push<NE>(st, f, head + i * NE, lab);
  }

  // wave merge (butterfly), then the four waves through LDS
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v = __shfl_xor(st.v, o, BMA_WAVE);
    const int vi = __shfl_xor(st.i, o, BMA_WAVE);
    best_merge(st, v, vi);
  }
  const int bad = __any(st.bad) ? 1 : 0;
  __shared__ float sv[kWaves];
  __shared__ int si[kWaves], sb[kWaves];
  const int wave = tid >> 6;
  if ((tid & 63) == 0) { sv[wave] = st.v; si[wave] = st.i; sb[wave] = bad; }
  __syncthreads();
  if (tid == 0) {
    Best r;
    r.v = sv[0]; r.i = si[0];
    int any_bad = sb[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) { best_merge(r, sv[w], si[w]); any_bad |= sb[w]; }
    float m = NAN;      // an out-of-range label, or a NaN anywhere in the row
    int hit = 0;
    if (lab >= 0) {
      const float zl = load_elem<DT>(base, lab);
      if (!any_bad) m = r.v - zl;
      hit = (zl > r.v || (zl == r.v && lab < r.i)) ? 1 : 0;   // the first argmax over all v is the label
    }
    ws[row] = m;
    reinterpret_cast<int32_t*>(ws)[BT + row] = r.i == kNone ? -1 : r.i;
    reinterpret_cast<int32_t*>(ws)[2 * BT + row] = hit;
  }
}

// loss[b] = (l[b,0] + ... + l[b,T-1]) / T with l = max(m, -kappa), summed in row order; match[b] = AND of the row hits.
__global__ __launch_bounds__(256) void margin_fold_kernel(const float* __restrict__ ws, int B, int T, int64_t BT,
                                                          float kappa, float* __restrict__ loss,
                                                          int32_t* __restrict__ match) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float acc = 0.0f;
  int all = 1;
  for (int t = 0; t < T; ++t) {
    const float m = ws[static_cast<int64_t>(b) * T + t];
    acc += m < -kappa ? -kappa : m;               // NaN stays NaN
    all &= reinterpret_cast<const int32_t*>(ws)[2 * BT + static_cast<int64_t>(b) * T + t];
  }
  loss[b] = acc / static_cast<float>(T);
  if (match) match[b] = all;
}

template <int DT>
__global__ __launch_bounds__(kThreads) void margin_dlogits_kernel(const int64_t* __restrict__ labels, int T, int V,
                                                                  const float* __restrict__ ws, int64_t BT, float kappa,
                                                                  void* __restrict__ dlogits, float g) {
  constexpr int ES = bma::elem_bytes<DT>::value, NE = 16 / ES;
  const int64_t row = blockIdx.x;
  const int tid = threadIdx.x;
  const bool active = ws[row] >= -kappa;           // equality passes, NaN does not (and then the label is in range)
  const int lab = active ? static_cast<int>(labels[row % T]) : -1;
  const int run = active ? reinterpret_cast<const int32_t*>(ws)[BT + row] : -1;
  const uint32_t at_lab = elem_bits<DT>(-g), at_run = elem_bits<DT>(g);
  char* obase = static_cast<char*>(dlogits) + row * V * ES;
  auto value = [&](int i) -> uint32_t { return i == lab ? at_lab : (i == run ? at_run : 0u); };
  auto put = [&](int i) {                          // one element, by the lane that owns it
    if (DT == BMA_F32) reinterpret_cast<uint32_t*>(obase)[i] = value(i);
    else reinterpret_cast<uint16_t*>(obase)[i] = static_cast<uint16_t>(value(i));
  };
  const int misfit = static_cast<int>(reinterpret_cast<uintptr_t>(obase) & 15);
  const int head = min(V, ((16 - misfit) & 15) / ES);
  const int nvec = (V - head) / NE;
  const int tail = head + nvec * NE;
  if (tid < head) put(tid);
  if (tid < V - tail) put(tail + tid);
  uint4_t* q = reinterpret_cast<uint4_t*>(obase + head * ES);
  // the vectors that hold the two non-zero elements (one vector may hold both)
  const int lv = (lab >= head && lab < tail) ? (lab - head) / NE : -1;
  const int rv = (run >= head && run < tail) ? (run - head) / NE : -1;
  for (int i = tid; i < nvec; i += kThreads) {
    uint32_t word[4] = {0u, 0u, 0u, 0u};
    if (i == lv || i == rv) {
#pragma unroll
      for (int k = 0; k < NE; ++k) {
        const uint32_t v = value(head + i * NE + k);
        if (DT == BMA_F32) word[k] = v;
        else word[k >> 1] |= v << (16 * (k & 1));
      }
    }
    uint4_t v;
    v.x = word[0]; v.y = word[1]; v.z = word[2]; v.w = word[3];
    q[i] = v;
  }
}

template <int DT>
int launch(const void* logits, int64_t ld_cand, int64_t ld_row, const int64_t* labels, int B, int T, int V, float kappa,
           float* ws, float* loss, int32_t* match, void* dlogits, float grad_scale, hipStream_t st) {
  constexpr int ES = bma::elem_bytes<DT>::value;
  const int64_t BT = static_cast<int64_t>(B) * T;
  const dim3 grid(static_cast<unsigned>(BT)), block(kThreads);
  BMA_PROF_BEGIN(BMA_K_MARGIN, st, static_cast<double>(BT) * V * ES);
  hipLaunchKernelGGL((margin_rows_kernel<DT>), grid, block, 0, st, logits, ld_cand, ld_row, labels, T, V, ws, BT);
  BMA_PROF_END(BMA_K_MARGIN, st);
  BMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(margin_fold_kernel, dim3((B + 255) / 256), dim3(256), 0, st, ws, B, T, BT, kappa, loss, match);
  BMA_LAUNCH_CHECK();
  if (dlogits) {
    const float g = grad_scale / static_cast<float>(T);
    BMA_PROF_BEGIN(BMA_K_MARGIN_DLOGITS, st, static_cast<double>(BT) * V * ES);
    hipLaunchKernelGGL((margin_dlogits_kernel<DT>), grid, block, 0, st, labels, T, V, ws, BT, kappa, dlogits, g);
    BMA_PROF_END(BMA_K_MARGIN_DLOGITS, st);
    BMA_LAUNCH_CHECK();
  }
  return BMA_OK;
}

}  // namespace

extern "C" size_t bma_margin_target_ws_bytes(int B, int T) {
  if (B < 0 || T < 0) return 0;
  return static_cast<size_t>(3) * static_cast<size_t>(B) * static_cast<size_t>(T) * 4;
}

extern "C" int bma_margin_target(const void* logits, int64_t ld_cand, int64_t ld_row, const int64_t* labels, int B,
                                 int T, int V, int dtype, float kappa, float* ws, float* loss, int32_t* match,
                                 void* dlogits, float grad_scale, void* stream) {
  if (B < 0 || T < 1 || V < 2 || ld_row < V || ld_cand < 0) return BMA_EINVAL;
  if (!(kappa >= 0.0f)) return BMA_EINVAL;                            // NaN fails the test; +inf: no clamp
  if (dtype != BMA_F32 && dtype != BMA_BF16 && dtype != BMA_F16) return BMA_EDTYPE;
  if (B == 0) return BMA_OK;
  if (!logits || !labels || !ws || !loss) return BMA_EINVAL;
  if (static_cast<int64_t>(B) * T > 0x7fffffffLL) return BMA_ELIMIT;
  const uintptr_t es = dtype == BMA_F32 ? 4 : 2;
  if (reinterpret_cast<uintptr_t>(logits) % es || reinterpret_cast<uintptr_t>(dlogits) % es ||
      reinterpret_cast<uintptr_t>(ws) % 4 || reinterpret_cast<uintptr_t>(loss) % 4 ||
      reinterpret_cast<uintptr_t>(match) % 4 || reinterpret_cast<uintptr_t>(labels) % 8)
    return BMA_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (dtype) {
    case BMA_F32: return launch<BMA_F32>(logits, ld_cand, ld_row, labels, B, T, V, kappa, ws, loss, match, dlogits, grad_scale, st);
    case BMA_BF16: return launch<BMA_BF16>(logits, ld_cand, ld_row, labels, B, T, V, kappa, ws, loss, match, dlogits, grad_scale, st);
    default: return launch<BMA_F16>(logits, ld_cand, ld_row, labels, B, T, V, kappa, ws, loss, match, dlogits, grad_scale, st);
  }
}
