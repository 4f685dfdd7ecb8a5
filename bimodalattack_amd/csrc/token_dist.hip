// a3b -- the embedding-distance term of the token top-k (opt-in, EngineOptions.token_dist_weight; contract in
//   include/bma.h):   out[i, v] = f32(grad[i, v]) + weight * || E[v, :] - E[ids[i], :] ||_2
// The one-hot gradient is a first-order estimate at the current token, whose error grows with the distance between the
// replacement's embedding and the current one (Faster-GCG's regulariser); the sum is what bma_mask_topk then ranks.
//
// One pass over the table per group of kRows = 32 suffix positions (a 20-token suffix: one pass).  The two bounds are of
// the same order at LLaVA width (263 MB of table; 20 * 32064 * 4096 subtract + FMA pairs), so the kernel must stream at
// full width AND keep the VALU fed:
//   - grid (ceil(V / 64), ceil(rows / 32)), 256 threads.  A workgroup owns 64 vocabulary rows and walks D in chunks of
//     256 bytes per row: the 64 x 256-byte tile is fetched with coalesced 16-byte loads (16 consecutive lanes cover one
//     row's 256 bytes) into REGISTERS one chunk ahead, and stored to LDS once the previous chunk's arithmetic is done --
//     the loads' latency sits under that arithmetic;
//   - the tile stays in the table's dtype in LDS, rows 272 bytes apart (one 16-byte slot of padding: lane l's
//     ds_read_b128 starts at bank 4l mod 64, conflict-free in every 16-lane group);
//   - lane l of every wave owns vocabulary row l of the tile, wave w owns suffix positions w, w + 4, w + 8, ...: one
//     accumulator per (position, row) in a register, no cross-lane reduction, one store per (i, v).  The number of
//     positions per wave is a template parameter (1..8), chosen per launch: 20 rows run 5, not 8;
//   - the current-token rows are the same for every lane of a wave, so they never enter a vector register or LDS: their
//     addresses are wave-uniform (readfirstlane), the compiler fetches them with SCALAR loads (16 bytes each, served by the
//     scalar cache and L2: 20 rows x 256 bytes per chunk, shared by every workgroup) and widens bf16 on the scalar unit;
//     the subtraction takes the scalar register as an operand.  The pieces are loaded one step ahead.
// Measured on an MI355X (tools/kernel_bench.py, bf16, 20 positions): 257 us at 32064 x 4096, 888 us at 262208 x 2560 -- 3 to
// 4 times the fp32 vector bound, far from the HBM one.  A variant that broadcast the current rows from LDS (one LDS cycle
// per value and wave) and builds without SLP packing of the fp32 arithmetic measured the same within 10 %: what holds the
// kernel back has not been found yet.
// Arithmetic: the difference form in fp32 on the exactly widened elements, acc += (e - x)^2 (the compiler may contract to
// FMA), sqrtf (correctly rounded: the build has no fast-math), weight * d + g.  A table row equal to the current one gives
// acc = +0 exactly, so the gradient passes through.

#include "bma_common.h"
#include "bma_profile.h"

namespace {

using bma::uint4_t;

constexpr int kRows = 32;                       // R of the contract: suffix positions per pass over the table
constexpr int kTile = 64;                       // vocabulary rows per workgroup = lanes per wave
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunkBytes = 256;                // per table row and step
constexpr int kPieces = kChunkBytes / 16;       // 16-byte pieces per row and chunk
constexpr int kTileStride = kChunkBytes + 16;   // bytes between tile rows in LDS
constexpr int kTileLoads = kTile * kPieces / kThreads;   // 4 pieces per thread

template <int DT> struct per_piece { static constexpr int value = 16 / bma::elem_bytes<DT>::value; };

template <int DT>
__device__ __forceinline__ void widen(const uint4_t w, float (&f)[per_piece<DT>::value]) {
  if (DT == BMA_F32) {
    f[0] = __uint_as_float(w.x); f[1] = __uint_as_float(w.y); f[2] = __uint_as_float(w.z); f[3] = __uint_as_float(w.w);
  } else {
    constexpr int NE = per_piece<DT>::value;
    f[0] = bma::unpack16<DT>(w.x, 0); f[1] = bma::unpack16<DT>(w.x, 1);
    f[2 % NE] = bma::unpack16<DT>(w.y, 0); f[3 % NE] = bma::unpack16<DT>(w.y, 1);
    f[4 % NE] = bma::unpack16<DT>(w.z, 0); f[5 % NE] = bma::unpack16<DT>(w.z, 1);
    f[6 % NE] = bma::unpack16<DT>(w.w, 0); f[7 % NE] = bma::unpack16<DT>(w.w, 1);
  }
}

template <int DT>
__device__ __forceinline__ float grad_at(const void* base, int64_t i) {
  if (DT == BMA_F32) return static_cast<const float*>(base)[i];
  const uint32_t h = static_cast<const uint16_t*>(base)[i];
  return DT == BMA_BF16 ? bma::bf16_bits_to_f32(h) : bma::f16_bits_to_f32(h);
}

// EDT: the table's dtype, GDT: the gradient's, NJ: suffix positions per wave (the group holds at most 4 * NJ).
template <int EDT, int GDT, int NJ>
__global__ __launch_bounds__(kThreads) void token_dist_kernel(const void* __restrict__ grad, int64_t ld_row, int rows, int V,
                                                              const void* __restrict__ emb, int64_t ld_emb, int D,
                                                              const int64_t* __restrict__ ids, float weight,
                                                              float* __restrict__ out, int64_t ld_out) {
  constexpr int ES = bma::elem_bytes<EDT>::value;
  constexpr int NE = per_piece<EDT>::value;            // elements per 16-byte piece
  __shared__ __attribute__((aligned(16))) unsigned char s_tile[kTile * kTileStride];
  __shared__ int64_t s_id[kRows];                      // the current token of each position; -1: none, or out of range

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int v0 = blockIdx.x * kTile;
  const int i0 = blockIdx.y * kRows;
  const int n = rows - i0 < kRows ? rows - i0 : kRows;  // positions of this group

  if (tid < kRows) {
    int64_t id = -1;
    if (tid < n) {
      id = ids[i0 + tid];
      if (id < 0 || id >= V) id = -1;                   // never read through
    }
    s_id[tid] = id;
  }
  __syncthreads();

  // what this thread stages: tile pieces t = tid + q * 256 -> (row t / 16, piece t % 16)
  const char* tsrc[kTileLoads];
#pragma unroll
  for (int q = 0; q < kTileLoads; ++q) {
    const int t = tid + q * kThreads, r = t / kPieces, p = t % kPieces;
    tsrc[q] = (v0 + r < V) ? static_cast<const char*>(emb) + (static_cast<int64_t>(v0 + r) * ld_emb) * ES + p * 16 : nullptr;
  }
  // the current-token rows of this wave's positions, wave-uniform.  A position without a token (beyond the group, or an id
  // outside the table) computes against row 0 -- a valid address, the id itself is never an index -- and is overwritten
  // (NaN) or not stored at the end.
  const int uwave = __builtin_amdgcn_readfirstlane(wave);
  const char* xrow[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int64_t id = s_id[uwave + kWaves * j];
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(id));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(static_cast<uint64_t>(id) >> 32));
    const int64_t uid = static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
    xrow[j] = static_cast<const char*>(emb) + ((uid >= 0 ? uid : 0) * ld_emb) * ES;
  }
  const int row_pieces = static_cast<int>((static_cast<int64_t>(D) * ES) / 16);   // D * ES is a multiple of 16
  const int p_mine = tid % kPieces;                     // (the same piece for every q: 256 is a multiple of 16)

  uint4_t treg[kTileLoads];
  auto fetch = [&](int piece0) {
    const bool in = piece0 + p_mine < row_pieces;
    const int64_t off = static_cast<int64_t>(piece0) * 16;
#pragma unroll
    for (int q = 0; q < kTileLoads; ++q) {
      uint4_t w = {0u, 0u, 0u, 0u};
      if (in && tsrc[q]) w = *reinterpret_cast<const uint4_t*>(tsrc[q] + off);
      treg[q] = w;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int q = 0; q < kTileLoads; ++q) {
      const int t = tid + q * kThreads, r = t / kPieces, p = t % kPieces;
      *reinterpret_cast<uint4_t*>(s_tile + r * kTileStride + p * 16) = treg[q];
    }
  };

  float acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = 0.0f;

  fetch(0);
  for (int piece0 = 0; piece0 < row_pieces; piece0 += kPieces) {
    __syncthreads();                                    // the previous chunk has been read by every wave
    stage();
    __syncthreads();
    if (piece0 + kPieces < row_pieces) fetch(piece0 + kPieces);
    const int np = row_pieces - piece0 < kPieces ? row_pieces - piece0 : kPieces;
    const unsigned char* trow = s_tile + lane * kTileStride;
    // the current rows' pieces one step ahead, in scalar registers: the scalar loads' latency sits under the arithmetic
    uint4_t xw[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) xw[j] = *reinterpret_cast<const uint4_t*>(xrow[j] + static_cast<int64_t>(piece0) * 16);
#pragma unroll 1
    for (int p = 0; p < np; ++p) {
      const int pn = p + 1 < np ? p + 1 : p;            // (the last step reloads its own piece: always inside the row)
      uint4_t xn[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) xn[j] = *reinterpret_cast<const uint4_t*>(xrow[j] + static_cast<int64_t>(piece0 + pn) * 16);
      float e[NE];
      widen<EDT>(*reinterpret_cast<const uint4_t*>(trow + p * 16), e);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        float x[NE];                                    // wave-uniform: scalar registers
        widen<EDT>(xw[j], x);
#pragma unroll
        for (int c = 0; c < NE; ++c) {
          const float d = e[c] - x[c];
          acc[j] += d * d;
        }
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) xw[j] = xn[j];
    }
  }

  const int v = v0 + lane;
  if (v < V) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int r = wave + kWaves * j;
      if (r < n) {                                        // (wave, not uwave: the same value, a vector compare)
        const int64_t i = i0 + r;
        const float g = grad_at<GDT>(grad, i * ld_row + v);
        const float d = sqrtf(acc[j]);
        out[i * ld_out + v] = s_id[r] >= 0 ? g + weight * d : __builtin_nanf("");
      }
    }
  }
}

template <int EDT, int GDT>
int launch(const void* grad, int64_t ld_row, int rows, int V, const void* emb, int64_t ld_emb, int D, const int64_t* ids,
           float weight, float* out, int64_t ld_out, hipStream_t st) {
  const int groups = (rows + kRows - 1) / kRows;
  const dim3 grid(static_cast<unsigned>((V + kTile - 1) / kTile), static_cast<unsigned>(groups));
  const int n_max = rows < kRows ? rows : kRows;        // the fullest group
  const int nj = (n_max + kWaves - 1) / kWaves;
  constexpr int ES = bma::elem_bytes<EDT>::value, GS = bma::elem_bytes<GDT>::value;
  BMA_PROF_BEGIN(BMA_K_TOKEN_DIST, st, static_cast<double>(groups) * V * D * ES + static_cast<double>(rows) * D * ES +
                                           static_cast<double>(rows) * V * (GS + 4.0));
#define BMA_TD(N)                                                                                                   \
  case N:                                                                                                           \
    hipLaunchKernelGGL((token_dist_kernel<EDT, GDT, N>), grid, dim3(kThreads), 0, st, grad, ld_row, rows, V, emb,  \
                       ld_emb, D, ids, weight, out, ld_out);                                                        \
    break
  switch (nj) {
    BMA_TD(1); BMA_TD(2); BMA_TD(3); BMA_TD(4); BMA_TD(5); BMA_TD(6); BMA_TD(7);
    default:
      hipLaunchKernelGGL((token_dist_kernel<EDT, GDT, 8>), grid, dim3(kThreads), 0, st, grad, ld_row, rows, V, emb, ld_emb,
                         D, ids, weight, out, ld_out);
  }
#undef BMA_TD
  BMA_PROF_END(BMA_K_TOKEN_DIST, st);
  BMA_LAUNCH_CHECK();
  return BMA_OK;
}

template <int EDT>
int launch_g(int gdtype, const void* grad, int64_t ld_row, int rows, int V, const void* emb, int64_t ld_emb, int D,
             const int64_t* ids, float weight, float* out, int64_t ld_out, hipStream_t st) {
  switch (gdtype) {
    case BMA_F32: return launch<EDT, BMA_F32>(grad, ld_row, rows, V, emb, ld_emb, D, ids, weight, out, ld_out, st);
    case BMA_BF16: return launch<EDT, BMA_BF16>(grad, ld_row, rows, V, emb, ld_emb, D, ids, weight, out, ld_out, st);
    default: return launch<EDT, BMA_F16>(grad, ld_row, rows, V, emb, ld_emb, D, ids, weight, out, ld_out, st);
  }
}

inline bool known(int dt) { return dt == BMA_F32 || dt == BMA_BF16 || dt == BMA_F16; }

}  // namespace

static_assert(kRows == BMA_TOKEN_DIST_ROWS, "the header states R");

extern "C" int bma_token_dist_score(const void* grad, int64_t ld_row, int rows, int V, int gdtype, const void* emb,
                                    int64_t ld_emb, int D, int edtype, const int64_t* ids, float weight, float* out,
                                    int64_t ld_out, void* stream) {
  if (rows < 1 || V < 1 || D < 1 || ld_row < V || ld_out < V || ld_emb < D) return BMA_EINVAL;
  if (!(weight >= 0.0f) || weight == __builtin_inff()) return BMA_EINVAL;      // NaN fails the first test
  if (!known(gdtype) || !known(edtype)) return BMA_EDTYPE;
  if (!grad || !emb || !ids || !out) return BMA_EINVAL;
  if ((rows + kRows - 1) / kRows > 65535) return BMA_ELIMIT;
  const int64_t es = edtype == BMA_F32 ? 4 : 2;
  const uintptr_t gs = gdtype == BMA_F32 ? 4 : 2;
  if (reinterpret_cast<uintptr_t>(emb) % 16 || (D * es) % 16 || (ld_emb * es) % 16 ||
      reinterpret_cast<uintptr_t>(grad) % gs || reinterpret_cast<uintptr_t>(out) % 4 ||
      reinterpret_cast<uintptr_t>(ids) % 8)
    return BMA_EALIGN;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (edtype) {
    case BMA_F32: return launch_g<BMA_F32>(gdtype, grad, ld_row, rows, V, emb, ld_emb, D, ids, weight, out, ld_out, st);
    case BMA_BF16: return launch_g<BMA_BF16>(gdtype, grad, ld_row, rows, V, emb, ld_emb, D, ids, weight, out, ld_out, st);
    default: return launch_g<BMA_F16>(gdtype, grad, ld_row, rows, V, emb, ld_emb, D, ids, weight, out, ld_out, st);
  }
}
