// a2, a2b, a2c -- the three target losses over the target slice, chosen by EngineOptions.loss_rule.  Contracts in
// include/bma.h; logits are B candidates x T rows x V columns, labels the T target ids.
//
// Shared machinery, each piece once:
//   RowSplit / row_split   a row that does not start or end on the 16-byte grid (small or odd V, ld_row > V, a block that
//                          starts off the grid) is [0, head) single elements, [head, tail) 16-byte vectors, [tail, V) single
//                          elements.
//   walk_row               one 256-thread workgroup reads one row once: head and tail elements by single lanes, the vectors
//                          with four 16-byte loads in flight per lane (4 KiB per wave per trip), then one vector per trip.
//                          Every chunk goes to the caller's push(f, N, first_index).
//   FirstMax               a (value, first index) maximum.  Ties go to the lower index at every level: inside a chunk, between
//                          a lane's chunks (which do not arrive in index order), in the xor butterfly across the wave and
//                          between the four waves through LDS.  fmaxf skips NaN; maxima start from -INFINITY, so a row of -inf
//                          keeps its first index.  The value equals z[index] up to the sign of a zero.
//   write_sparse_row       a write-only row of dlogits: zeros as 16-byte vectors, head and tail elements by single lanes, and
//                          up to two non-zero elements (they may share a vector, or sit one in the head and one in the tail).
//                          Every element is written by exactly one lane.
//   target_fold_kernel     a tiny launch folds the T row terms of a candidate in row order (bitwise reproducible, no atomics)
//                          and ANDs the row hits.
//   run                    one argument check and one dtype dispatch for the three entry points.
//
// a2 -- cross-entropy (the default)
//   candidate scoring: reference bimodal_attack.py:1289-1306 (CE "none" -> view(B,T).mean(-1), early-stop argmax test)
//   gradient pass:     reference bimodal_attack.py:1006-1012 (mean CE; autograd supplies (softmax - onehot)/T, produced here
//                      directly)
//   HBM-bound: the B*T rows of V logits are read exactly once (657 MB per step at B=512, T=20, V=32064, bf16), B*T = 10,240
//   workgroups >> 256 CUs.  Each lane keeps an online (max, sum-of-exp) pair in fp32, so the row maximum never needs a second
//   pass; the pairs are merged like the FirstMax that rides along for the early-stop test.  Rows off the 16-byte grid are read
//   element by element, all of them by tid stride (the VEC = false path: its own summation order).  ce_dlogits_kernel is
//   dense: it reads the logits again.
//   ws (3*B*T 4-byte words): [0,BT) row loss f32 | [BT,2BT) row argmax==label i32 | [2BT,3BT) row logsumexp f32 (consumed by
//   the dlogits pass).
//
// a2b -- nanoGCG's mellowmax (opt-in, loss_rule = "mellowmax")
//   the function: reference bimodalattack/utils.py:35-36 (shipped, never called there), applied as nanoGCG applies it: to the
//   NEGATED RAW target logits of a candidate, no softmax over the vocabulary.
//     a_j  = alpha * -float(z[j, y_j])                         j = 0..T-1
//     m    = max_j a_j, replaced by 0 when it is +-inf         (torch.logsumexp's rule)
//     s    = sum_j exp(a_j - m)
//     loss = ((log(s) + m) - log(T)) / alpha
//     w_j  = exp(a_j - m) / s                                  d loss / d z[j, y_j] = -w_j
//   Loss pass: one element per ROW is read (B*T gathers; the V columns are never streamed), so the pass is latency-, not
//   bandwidth-bound: a wave per candidate while T fits one sweep of a wave (four candidates per workgroup), a 256-thread
//   workgroup per candidate beyond that.  Each lane folds its rows j = lane, lane + n, ... in that order, the lanes are merged
//   by an xor butterfly (every lane ends with the same bits) and the four waves in wave order through LDS: the order is fixed,
//   two calls on one input are bitwise equal, there are no atomics.  NaN needs no flag: fmaxf skips it, exp keeps it, so it
//   reaches s and from there the loss and every weight of the candidate.
//   dlogits pass: write_sparse_row with -w_j * grad_scale at the label (657 MB at B=512, T=20, V=32064, bf16).
//   ws (B*T floats): w.
//
// a2c -- the Carlini-Wagner margin (opt-in, loss_rule = "margin")
//     o_j  = max over v != y_j of z_v,  i_j = the FIRST index v != y_j with z_v == o_j   (o_j = z[i_j])
//     m_j  = o_j - z[y_j]
//     loss = (sum_j max(m_j, -kappa)) / T                     summed in row order
//     a_j  = m_j >= -kappa                                    dlogits: -a_j*g at y_j, +a_j*g at i_j, g = grad_scale / T
//     match = every row's first argmax over ALL v is its label (bma_ce_target's early-stop test)
//   Row pass: HBM-bound like ce_rows_kernel, with walk_row on the row's real split, so one kernel serves every alignment.  A
//   lane keeps ONE FirstMax, over v != y: the label's element is taken out of the maximum as it goes by.  The argmax over all
//   v that the early-stop test needs follows from that pair and z[y_j], which the margin reads anyway: it is y_j exactly when
//   z[y_j] > o_j, or z[y_j] == o_j with y_j < i_j.  o_j is read back as z[i_j] by the lane that writes the row's result, so
//   a zero keeps its sign.  A NaN flag rides along; it is taken before the label is taken out, so a NaN at the label counts.
//   dlogits pass: write_sparse_row with two non-zero elements per active row.
//   ws (3*B*T 4-byte words): [0,BT) m f32 | [BT,2BT) i int32 (-1: none) | [2BT,3BT) row hit int32.

#include <type_traits>

#include "bma_common.h"
#include "bma_profile.h"

namespace {

using bma::elem_bits;
using bma::load_elem;
using bma::uint4_t;
using bma::unpack;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / BMA_WAVE;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kNegBig = -3.0e38f;

template <int N>
using Count = std::integral_constant<int, N>;

// ---------------------------------------------------------------------------------------------------------- shared pieces
struct RowSplit {
  int head, nvec, tail;   // [0, head) up to the first 16-byte boundary, [head, tail) as nvec vectors, [tail, V) the rest
};

template <int DT>
__device__ __forceinline__ RowSplit row_split(const void* base, int V) {
  constexpr int ES = bma::elem_bytes<DT>::value, NE = 16 / ES;
  const int misfit = static_cast<int>(reinterpret_cast<uintptr_t>(base) & 15);
  RowSplit s;
  s.head = min(V, ((16 - misfit) & 15) / ES);
  s.nvec = (V - s.head) / NE;
  s.tail = s.head + s.nvec * NE;
  return s;
}

// The workgroup's one read of the row at `base`: push(f, Count<N>, first_index) for every chunk of N consecutive elements.
template <int DT, class Push>
__device__ __forceinline__ void walk_row(const char* base, int V, const RowSplit& sp, Push&& push) {
  constexpr int ES = bma::elem_bytes<DT>::value, NE = 16 / ES;
  const int tid = threadIdx.x;
  if (tid < sp.head) {
    float f[1] = {load_elem<DT>(base, tid)};
    push(f, Count<1>{}, tid);
  }
  if (tid < V - sp.tail) {
    float f[1] = {load_elem<DT>(base, sp.tail + tid)};
    push(f, Count<1>{}, sp.tail + tid);
  }
  const uint4_t* p = reinterpret_cast<const uint4_t*>(base + sp.head * ES);
  int i = tid;
  for (; i + 3 * kThreads < sp.nvec; i += 4 * kThreads) {
    const uint4_t w0 = p[i], w1 = p[i + kThreads], w2 = p[i + 2 * kThreads], w3 = p[i + 3 * kThreads];
    float f[NE];
    unpack<DT>(w0, f); push(f, Count<NE>{}, sp.head + i * NE);
    unpack<DT>(w1, f); push(f, Count<NE>{}, sp.head + (i + kThreads) * NE);
    unpack<DT>(w2, f); push(f, Count<NE>{}, sp.head + (i + 2 * kThreads) * NE);
    unpack<DT>(w3, f); push(f, Count<NE>{}, sp.head + (i + 3 * kThreads) * NE);
  }
  for (; i < sp.nvec; i += kThreads) {
    float f[NE];
    unpack<DT>(p[i], f);
    push(f, Count<NE>{}, sp.head + i * NE);
  }
}

template <int N>
__device__ __forceinline__ float chunk_max(const float* f) {
  float cm = f[0];
#pragma unroll
  for (int j = 1; j < N; ++j) cm = fmaxf(cm, f[j]);
  return cm;
}

struct FirstMax {
  float v;   // the best value so far (NaN skipped)
  int i;     // its first index; kNone: nothing seen yet
  static constexpr int kNone = 0x7fffffff;
  struct Waves { float v[kWaves]; int i[kWaves]; };   // the LDS of the cross-wave merge

  __device__ __forceinline__ void init() { v = -INFINITY; i = kNone; }
  __device__ __forceinline__ void merge(float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  // N consecutive elements starting at index `first`, cm = chunk_max<N>(f)
  template <int N>
  __device__ __forceinline__ void push(const float* f, float cm, int first) {
    if (cm > v || (cm == v && first < i)) {   // this lane's chunks are not monotone in index
#pragma unroll
      for (int j = N - 1; j >= 0; --j)
        if (f[j] == cm) i = first + j;
      v = cm;   // equal to f[i], up to the sign of a zero
    }
  }
  __device__ __forceinline__ void butterfly() {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, BMA_WAVE);
      const int oi = __shfl_xor(i, o, BMA_WAVE);
      merge(ov, oi);
    }
  }
  // after butterfly(): lane 0 of every wave put()s, the workgroup syncs, one lane take()s the four waves in wave order
  __device__ __forceinline__ void put(Waves& lds, int wave) const { lds.v[wave] = v; lds.i[wave] = i; }
  __device__ __forceinline__ void take(const Waves& lds) {
    v = lds.v[0]; i = lds.i[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) merge(lds.v[w], lds.i[w]);
  }
};

// One row of dlogits at `obase`: b0 at element i0, b1 at element i1 (-1: none; i0 != i1), +0 everywhere else.
template <int DT>
__device__ __forceinline__ void write_sparse_row(char* obase, int V, int i0, uint32_t b0, int i1, uint32_t b1) {
  constexpr int ES = bma::elem_bytes<DT>::value, NE = 16 / ES;
  const int tid = threadIdx.x;
  auto value = [&](int i) -> uint32_t { return i == i0 ? b0 : (i == i1 ? b1 : 0u); };
  auto put = [&](int i) {                          // one element, by the lane that owns it
    if (DT == BMA_F32) reinterpret_cast<uint32_t*>(obase)[i] = value(i);
    else reinterpret_cast<uint16_t*>(obase)[i] = static_cast<uint16_t>(value(i));
  };
  const RowSplit sp = row_split<DT>(obase, V);
  if (tid < sp.head) put(tid);
  if (tid < V - sp.tail) put(sp.tail + tid);
  uint4_t* q = reinterpret_cast<uint4_t*>(obase + sp.head * ES);
  // the vectors that hold the non-zero elements (one vector may hold both)
  const int v0 = (i0 >= sp.head && i0 < sp.tail) ? (i0 - sp.head) / NE : -1;
  const int v1 = (i1 >= sp.head && i1 < sp.tail) ? (i1 - sp.head) / NE : -1;
  for (int i = tid; i < sp.nvec; i += kThreads) {
    uint32_t word[4] = {0u, 0u, 0u, 0u};
    if (i == v0 || i == v1) {
#pragma unroll
      for (int k = 0; k < NE; ++k) {
        const uint32_t v = value(sp.head + i * NE + k);
        if (DT == BMA_F32) word[k] = v;
        else word[k >> 1] |= v << (16 * (k & 1));
      }
    }
    uint4_t v;
    v.x = word[0]; v.y = word[1]; v.z = word[2]; v.w = word[3];
    q[i] = v;
  }
}

// loss[b] = (l[b,0] + ... + l[b,T-1]) / T, summed in row order, with l = CLAMP ? max(row, -kappa) : row;
// match[b] = AND of the row hits.
template <bool CLAMP>
__global__ __launch_bounds__(256) void target_fold_kernel(const float* __restrict__ rows, const int32_t* __restrict__ hits,
                                                          int B, int T, float kappa, float* __restrict__ loss,
                                                          int32_t* __restrict__ match) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float acc = 0.0f;
  int all = 1;
  for (int t = 0; t < T; ++t) {
    const float m = rows[static_cast<int64_t>(b) * T + t];
    acc += (CLAMP && m < -kappa) ? -kappa : m;    // NaN stays NaN
    all &= hits[static_cast<int64_t>(b) * T + t];
  }
  loss[b] = acc / static_cast<float>(T);
  if (match) match[b] = all;
}

// ---------------------------------------------------------------------------------------------------- a2: cross-entropy
struct MaxSum {
  float m, s;   // running maximum, sum of exp(x - m)
  template <int N>
  __device__ __forceinline__ void push(const float* f, float cm) {
    const float mn = fmaxf(m, cm);
    float acc = s * __builtin_amdgcn_exp2f((m - mn) * kLog2e);
#pragma unroll
    for (int j = 0; j < N; ++j) acc += __builtin_amdgcn_exp2f((f[j] - mn) * kLog2e);
    s = acc;
    m = mn;
  }
  __device__ __forceinline__ void merge(float om, float os) {
    const float mn = fmaxf(m, om);
    s = s * __builtin_amdgcn_exp2f((m - mn) * kLog2e) + os * __builtin_amdgcn_exp2f((om - mn) * kLog2e);
    m = mn;
  }
};

// One workgroup per row.  VEC: rows are 16-byte aligned and V % NE == 0.  ARGMAX = false (no `match` wanted: the gradient
// pass) does no argmax work.
template <int DT, bool VEC, bool ARGMAX>
__global__ __launch_bounds__(kThreads) void ce_rows_kernel(const void* __restrict__ logits, int64_t ld_cand,
                                                           int64_t ld_row, const int64_t* __restrict__ labels,
                                                           int T, int V, float* __restrict__ ws, int64_t BT) {
  const int64_t row = blockIdx.x;
  const int b = static_cast<int>(row / T), t = static_cast<int>(row % T);
  const int64_t off = static_cast<int64_t>(b) * ld_cand + static_cast<int64_t>(t) * ld_row;
  const char* base = static_cast<const char*>(logits) + off * bma::elem_bytes<DT>::value;
  const int tid = threadIdx.x;

  MaxSum st;
  st.m = kNegBig; st.s = 0.0f;
  FirstMax best;
  best.init();
  auto push = [&](float* f, auto n, int first) {
    constexpr int N = decltype(n)::value;
    const float cm = chunk_max<N>(f);
    st.push<N>(f, cm);
    if (ARGMAX) best.push<N>(f, cm, first);
  };
  if (VEC) {
    const RowSplit whole = {0, V / (16 / bma::elem_bytes<DT>::value), V};
    walk_row<DT>(base, V, whole, push);
  } else {
    for (int i = tid; i < V; i += kThreads) {
      float f[1] = {load_elem<DT>(base, i)};
      push(f, Count<1>{}, i);
    }
  }

  // wave merge (butterfly), then the four waves through LDS
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m = __shfl_xor(st.m, o, BMA_WAVE), s = __shfl_xor(st.s, o, BMA_WAVE);
    st.merge(m, s);
  }
  if (ARGMAX) best.butterfly();
  __shared__ float sm[kWaves][2];
  __shared__ FirstMax::Waves sbest;
  const int wave = tid >> 6;
  if ((tid & 63) == 0) {
    sm[wave][0] = st.m; sm[wave][1] = st.s;
    if (ARGMAX) best.put(sbest, wave);
  }
  __syncthreads();
  if (tid == 0) {
    st.m = sm[0][0]; st.s = sm[0][1];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) st.merge(sm[w][0], sm[w][1]);
    if (ARGMAX) best.take(sbest);
    const int64_t lab = labels[t];
    const float lse = st.m + __logf(st.s);
    float xl = NAN;  // an out-of-range label poisons the loss instead of reading out of bounds
    if (lab >= 0 && lab < V) xl = load_elem<DT>(base, lab);
    ws[row] = lse - xl;
    reinterpret_cast<int32_t*>(ws)[BT + row] = ARGMAX ? (best.i == static_cast<int>(lab) ? 1 : 0) : 0;
    ws[2 * BT + row] = lse;
  }
}

// dlogits[row, v] = (exp(x - lse) - [v == label]) * scale   (scale = grad_scale / T)
template <int DT, bool VEC>
__global__ __launch_bounds__(kThreads) void ce_dlogits_kernel(const void* __restrict__ logits, int64_t ld_cand,
                                                              int64_t ld_row, const int64_t* __restrict__ labels,
                                                              int T, int V, const float* __restrict__ ws, int64_t BT,
                                                              void* __restrict__ dlogits, float scale) {
  const int64_t row = blockIdx.x;
  const int b = static_cast<int>(row / T), t = static_cast<int>(row % T);
  const int64_t off = static_cast<int64_t>(b) * ld_cand + static_cast<int64_t>(t) * ld_row;
  const char* base = static_cast<const char*>(logits) + off * bma::elem_bytes<DT>::value;
  char* obase = static_cast<char*>(dlogits) + row * V * bma::elem_bytes<DT>::value;
  const float lse = ws[2 * BT + row];
  const int lab = static_cast<int>(labels[t]);
  const int tid = threadIdx.x;
  if (VEC) {
    constexpr int NE = 16 / bma::elem_bytes<DT>::value;
    const uint4_t* p = reinterpret_cast<const uint4_t*>(base);
    uint4_t* q = reinterpret_cast<uint4_t*>(obase);
    const int nvec = V / NE;
    for (int i = tid; i < nvec; i += kThreads) {
      float f[NE];
      unpack<DT>(p[i], f);
#pragma unroll
      for (int j = 0; j < NE; ++j) {
        const float pr = __builtin_amdgcn_exp2f((f[j] - lse) * kLog2e);
        f[j] = (pr - ((i * NE + j) == lab ? 1.0f : 0.0f)) * scale;
      }
      uint4_t w;
      if (DT == BMA_F32) {
        w.x = __float_as_uint(f[0]); w.y = __float_as_uint(f[1]);
        w.z = __float_as_uint(f[2]); w.w = __float_as_uint(f[3]);
      } else {
        w.x = bma::pack16<DT>(f[0], f[1]); w.y = bma::pack16<DT>(f[2], f[3]);
        w.z = bma::pack16<DT>(f[4 % NE], f[5 % NE]); w.w = bma::pack16<DT>(f[6 % NE], f[7 % NE]);
      }
      q[i] = w;
    }
  } else {
    for (int i = tid; i < V; i += kThreads) {
      const float x = load_elem<DT>(base, i);
      const float v = (__builtin_amdgcn_exp2f((x - lse) * kLog2e) - (i == lab ? 1.0f : 0.0f)) * scale;
      if (DT == BMA_F32) reinterpret_cast<uint32_t*>(obase)[i] = elem_bits<DT>(v);
      else reinterpret_cast<uint16_t*>(obase)[i] = static_cast<uint16_t>(elem_bits<DT>(v));
    }
  }
}

// ------------------------------------------------------------------------------------------------------- a2b: mellowmax
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
  const int64_t row = blockIdx.x;
  const int64_t lab64 = labels[row % T];
  const int lab = (lab64 >= 0 && lab64 < V) ? static_cast<int>(lab64) : -1;      // out of range: the row is all zeros
  char* obase = static_cast<char*>(dlogits) + row * V * bma::elem_bytes<DT>::value;
  write_sparse_row<DT>(obase, V, lab, elem_bits<DT>(-ws[row] * grad_scale), -1, 0u);
}

// ---------------------------------------------------------------------------------------------------------- a2c: margin
template <int DT>
__global__ __launch_bounds__(kThreads) void margin_rows_kernel(const void* __restrict__ logits, int64_t ld_cand,
                                                               int64_t ld_row, const int64_t* __restrict__ labels,
                                                               int T, int V, float* __restrict__ ws, int64_t BT) {
  const int64_t row = blockIdx.x;
  const int b = static_cast<int>(row / T), t = static_cast<int>(row % T);
  const int64_t off = static_cast<int64_t>(b) * ld_cand + static_cast<int64_t>(t) * ld_row;
  const char* base = static_cast<const char*>(logits) + off * bma::elem_bytes<DT>::value;
  const int tid = threadIdx.x;
  const int64_t lab64 = labels[t];
  const int lab = (lab64 >= 0 && lab64 < V) ? static_cast<int>(lab64) : -1;   // out of range: never read through

  FirstMax best;      // over v != y
  best.init();
  bool bad = false;   // a NaN went by (the label's element included)
  walk_row<DT>(base, V, row_split<DT>(base, V), [&](float* f, auto n, int first) {
    constexpr int N = decltype(n)::value;
    bool nan = false;
#pragma unroll
    for (int j = 0; j < N; ++j) nan |= f[j] != f[j];
    bad |= nan;
    const unsigned k = static_cast<unsigned>(lab - first);
    if (k < static_cast<unsigned>(N)) {             // the label's own chunk: one lane of the row, once
#pragma unroll
      for (int j = 0; j < N; ++j)
        if (j == static_cast<int>(k)) f[j] = NAN;   // skipped by fmaxf, equal to nothing
    }
    best.push<N>(f, chunk_max<N>(f), first);
  });

  // wave merge (butterfly), then the four waves through LDS
  best.butterfly();
  const int wave_bad = __any(bad) ? 1 : 0;
  __shared__ FirstMax::Waves sbest;
  __shared__ int sbad[kWaves];
  const int wave = tid >> 6;
  if ((tid & 63) == 0) { best.put(sbest, wave); sbad[wave] = wave_bad; }
  __syncthreads();
  if (tid == 0) {
    best.take(sbest);
    int any_bad = sbad[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) any_bad |= sbad[w];
    float m = NAN;      // an out-of-range label, or a NaN anywhere in the row
    int hit = 0;
    if (lab >= 0) {
      const float zl = load_elem<DT>(base, lab);
      const float o = best.i == FirstMax::kNone ? best.v : load_elem<DT>(base, best.i);   // z[i_j]: the sign of a zero
      if (!any_bad) m = o - zl;
      hit = (zl > o || (zl == o && lab < best.i)) ? 1 : 0;   // the first argmax over all v is the label
    }
    ws[row] = m;
    reinterpret_cast<int32_t*>(ws)[BT + row] = best.i == FirstMax::kNone ? -1 : best.i;
    reinterpret_cast<int32_t*>(ws)[2 * BT + row] = hit;
  }
}

template <int DT>
__global__ __launch_bounds__(kThreads) void margin_dlogits_kernel(const int64_t* __restrict__ labels, int T, int V,
                                                                  const float* __restrict__ ws, int64_t BT, float kappa,
                                                                  void* __restrict__ dlogits, float g) {
  const int64_t row = blockIdx.x;
  const bool active = ws[row] >= -kappa;           // equality passes, NaN does not (and then the label is in range)
  const int lab = active ? static_cast<int>(labels[row % T]) : -1;
  const int run = active ? reinterpret_cast<const int32_t*>(ws)[BT + row] : -1;
  char* obase = static_cast<char*>(dlogits) + row * V * bma::elem_bytes<DT>::value;
  write_sparse_row<DT>(obase, V, lab, elem_bits<DT>(-g), run, elem_bits<DT>(g));
}

// ------------------------------------------------------------------------------------------------------------ host side
struct Call {
  const void* logits;
  int64_t ld_cand, ld_row;
  const int64_t* labels;
  int B, T, V;
  float* ws;
  float* loss;
  int32_t* match;
  void* dlogits;
  float grad_scale;
  hipStream_t st;
  int64_t BT() const { return static_cast<int64_t>(B) * T; }
  dim3 rows() const { return dim3(static_cast<unsigned>(BT())); }
  const int32_t* ws_i32(int third) const { return reinterpret_cast<const int32_t*>(ws) + third * BT(); }
};

// The checks of all three entry points, in this order: ranges and the rule's own parameter (`param_ok`), dtype, B == 0
// (nothing to do), null pointers, the B*T limit, alignment.  Then launch(Count<dtype>).
template <class Launch>
int run(const Call& c, int dtype, int min_V, bool param_ok, Launch&& launch) {
  if (c.B < 0 || c.T < 1 || c.V < min_V || c.ld_row < c.V || c.ld_cand < 0 || !param_ok) return BMA_EINVAL;
  if (dtype != BMA_F32 && dtype != BMA_BF16 && dtype != BMA_F16) return BMA_EDTYPE;
  if (c.B == 0) return BMA_OK;
  if (!c.logits || !c.labels || !c.ws || !c.loss) return BMA_EINVAL;
  if (c.BT() > 0x7fffffffLL) return BMA_ELIMIT;
  const uintptr_t es = dtype == BMA_F32 ? 4 : 2;
  if (reinterpret_cast<uintptr_t>(c.logits) % es || reinterpret_cast<uintptr_t>(c.dlogits) % es ||
      reinterpret_cast<uintptr_t>(c.ws) % 4 || reinterpret_cast<uintptr_t>(c.loss) % 4 ||
      reinterpret_cast<uintptr_t>(c.match) % 4 || reinterpret_cast<uintptr_t>(c.labels) % 8)
    return BMA_EALIGN;
  switch (dtype) {
    case BMA_F32: return launch(Count<BMA_F32>{});
    case BMA_BF16: return launch(Count<BMA_BF16>{});
    default: return launch(Count<BMA_F16>{});
  }
}

size_t ws_bytes(int B, int T, int words_per_row) {
  if (B < 0 || T < 0) return 0;
  return static_cast<size_t>(words_per_row) * static_cast<size_t>(B) * static_cast<size_t>(T) * 4;
}

template <int DT>
int launch_ce(const Call& c) {
  constexpr int ES = bma::elem_bytes<DT>::value;
  const int64_t BT = c.BT();
  const bool vec = (reinterpret_cast<uintptr_t>(c.logits) % 16 == 0) && ((c.ld_cand * ES) % 16 == 0) &&
                   ((c.ld_row * ES) % 16 == 0) && ((static_cast<int64_t>(c.V) * ES) % 16 == 0);
  const dim3 block(kThreads);
  const bool am = c.match != nullptr;
#define BMA_CE_GO(VEC_, AM_)                                                                                        \
  hipLaunchKernelGGL((ce_rows_kernel<DT, VEC_, AM_>), c.rows(), block, 0, c.st, c.logits, c.ld_cand, c.ld_row, c.labels, \
                     c.T, c.V, c.ws, BT)
  const int prof_slot = c.B > 1 ? BMA_K_CE_ROWS : BMA_K_CE_ROWS_B1;
  BMA_PROF_BEGIN(prof_slot, c.st, static_cast<double>(BT) * c.V * ES);
  if (vec) { if (am) BMA_CE_GO(true, true); else BMA_CE_GO(true, false); }
  else     { if (am) BMA_CE_GO(false, true); else BMA_CE_GO(false, false); }
#undef BMA_CE_GO
  BMA_PROF_END(prof_slot, c.st);
  BMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(target_fold_kernel<false>, dim3((c.B + 255) / 256), dim3(256), 0, c.st, c.ws, c.ws_i32(1), c.B, c.T,
                     0.0f, c.loss, c.match);
  BMA_LAUNCH_CHECK();
  if (c.dlogits) {
    const bool ovec = vec && (reinterpret_cast<uintptr_t>(c.dlogits) % 16 == 0);
    const float scale = c.grad_scale / static_cast<float>(c.T);
    BMA_PROF_BEGIN(BMA_K_CE_DLOGITS, c.st, 2.0 * static_cast<double>(BT) * c.V * ES);
    if (ovec)
      hipLaunchKernelGGL((ce_dlogits_kernel<DT, true>), c.rows(), block, 0, c.st, c.logits, c.ld_cand, c.ld_row, c.labels,
                         c.T, c.V, c.ws, BT, c.dlogits, scale);
    else
      hipLaunchKernelGGL((ce_dlogits_kernel<DT, false>), c.rows(), block, 0, c.st, c.logits, c.ld_cand, c.ld_row, c.labels,
                         c.T, c.V, c.ws, BT, c.dlogits, scale);
    BMA_PROF_END(BMA_K_CE_DLOGITS, c.st);
    BMA_LAUNCH_CHECK();
  }
  return BMA_OK;
}

template <int DT>
int launch_mellowmax(const Call& c, float alpha) {
  constexpr int ES = bma::elem_bytes<DT>::value;
  const int64_t BT = c.BT();
  BMA_PROF_BEGIN(BMA_K_MELLOWMAX, c.st, static_cast<double>(BT) * (ES + 8 + 4) + 4.0 * c.B);
  if (c.T <= BMA_WAVE)
    hipLaunchKernelGGL((mellowmax_loss_kernel<DT, false>), dim3((c.B + kWaves - 1) / kWaves), dim3(kThreads), 0, c.st,
                       c.logits, c.ld_cand, c.ld_row, c.labels, c.B, c.T, c.V, alpha, c.ws, c.loss);
  else
    hipLaunchKernelGGL((mellowmax_loss_kernel<DT, true>), dim3(c.B), dim3(kThreads), 0, c.st, c.logits, c.ld_cand, c.ld_row,
                       c.labels, c.B, c.T, c.V, alpha, c.ws, c.loss);
  BMA_PROF_END(BMA_K_MELLOWMAX, c.st);
  BMA_LAUNCH_CHECK();
  if (c.dlogits) {
    BMA_PROF_BEGIN(BMA_K_MELLOWMAX_DLOGITS, c.st, static_cast<double>(BT) * c.V * ES);
    hipLaunchKernelGGL((mellowmax_dlogits_kernel<DT>), c.rows(), dim3(kThreads), 0, c.st, c.labels, c.T, c.V, c.ws,
                       c.dlogits, c.grad_scale);
    BMA_PROF_END(BMA_K_MELLOWMAX_DLOGITS, c.st);
    BMA_LAUNCH_CHECK();
  }
  return BMA_OK;
}

template <int DT>
int launch_margin(const Call& c, float kappa) {
  constexpr int ES = bma::elem_bytes<DT>::value;
  const int64_t BT = c.BT();
  const dim3 block(kThreads);
  BMA_PROF_BEGIN(BMA_K_MARGIN, c.st, static_cast<double>(BT) * c.V * ES);
  hipLaunchKernelGGL((margin_rows_kernel<DT>), c.rows(), block, 0, c.st, c.logits, c.ld_cand, c.ld_row, c.labels, c.T, c.V,
                     c.ws, BT);
  BMA_PROF_END(BMA_K_MARGIN, c.st);
  BMA_LAUNCH_CHECK();
  hipLaunchKernelGGL(target_fold_kernel<true>, dim3((c.B + 255) / 256), dim3(256), 0, c.st, c.ws, c.ws_i32(2), c.B, c.T,
                     kappa, c.loss, c.match);
  BMA_LAUNCH_CHECK();
  if (c.dlogits) {
    const float g = c.grad_scale / static_cast<float>(c.T);
    BMA_PROF_BEGIN(BMA_K_MARGIN_DLOGITS, c.st, static_cast<double>(BT) * c.V * ES);
    hipLaunchKernelGGL((margin_dlogits_kernel<DT>), c.rows(), block, 0, c.st, c.labels, c.T, c.V, c.ws, BT, kappa,
                       c.dlogits, g);
    BMA_PROF_END(BMA_K_MARGIN_DLOGITS, c.st);
    BMA_LAUNCH_CHECK();
  }
  return BMA_OK;
}

}  // namespace

extern "C" size_t bma_ce_target_ws_bytes(int B, int T) { return ws_bytes(B, T, 3); }
extern "C" size_t bma_mellowmax_target_ws_bytes(int B, int T) { return ws_bytes(B, T, 1); }
extern "C" size_t bma_margin_target_ws_bytes(int B, int T) { return ws_bytes(B, T, 3); }

extern "C" int bma_ce_target(const void* logits, int64_t ld_cand, int64_t ld_row, const int64_t* labels, int B,
                             int T, int V, int dtype, float* ws, float* loss, int32_t* match, void* dlogits,
                             float grad_scale, void* stream) {
  const Call c = {logits, ld_cand, ld_row, labels, B, T, V, ws, loss, match, dlogits, grad_scale,
                  static_cast<hipStream_t>(stream)};
  return run(c, dtype, 1, true, [&](auto dt) { return launch_ce<decltype(dt)::value>(c); });
}

extern "C" int bma_mellowmax_target(const void* logits, int64_t ld_cand, int64_t ld_row, const int64_t* labels, int B,
                                    int T, int V, int dtype, float alpha, float* ws, float* loss, void* dlogits,
                                    float grad_scale, void* stream) {
  const Call c = {logits, ld_cand, ld_row, labels, B, T, V, ws, loss, nullptr, dlogits, grad_scale,
                  static_cast<hipStream_t>(stream)};
  const bool alpha_ok = alpha > 0.0f && alpha != INFINITY;            // NaN fails the first test
  return run(c, dtype, 1, alpha_ok, [&](auto dt) { return launch_mellowmax<decltype(dt)::value>(c, alpha); });
}

extern "C" int bma_margin_target(const void* logits, int64_t ld_cand, int64_t ld_row, const int64_t* labels, int B,
                                 int T, int V, int dtype, float kappa, float* ws, float* loss, int32_t* match,
                                 void* dlogits, float grad_scale, void* stream) {
  const Call c = {logits, ld_cand, ld_row, labels, B, T, V, ws, loss, match, dlogits, grad_scale,
                  static_cast<hipStream_t>(stream)};
  const bool kappa_ok = kappa >= 0.0f;                                // NaN fails the test; +inf: no clamp
  return run(c, dtype, 2, kappa_ok, [&](auto dt) { return launch_margin<decltype(dt)::value>(c, kappa); });
}
