// Embedding, float32: the forward row gather out[t] = table[id[t]] and the backward scatter-sum
// dtable[v] = sum of dy[t] over the tokens t with id[t] == v, for n = B*T tokens, a [V, D] table, D a multiple of 4
// from 4 to 512.  No float atomics: every dtable element is summed by ONE thread in increasing t from 0, so the
// result is a function of the ids alone and equals numpy's add.at on a float32 zero array bit for bit.
//
// Ids: float32 (the f32 plan's input ring; truncated toward zero, as Keras's cast to int32, exact up to
// V = 2^24) or int32 by a flag.  An id outside [0, V) reads as a zero row and takes part in no gradient; no address
// is ever formed from it (ids are tested first, a refused id is replaced by -1 and only tested again).
//
// * Forward: a wave's lanes run over the D/4 float4 columns of a row first and over tokens second, so with
//   D/4 < 64 a wave covers 64 / (D/4) tokens per pass (256/D) and every access is a full 16-byte one.  The ids of a
//   pass are loaded once, one per lane, and handed to the token's lanes by a lane shuffle.
// * Backward, an owner scan without a sort: a 256-thread workgroup owns RB = min(64, 8192/D) consecutive table rows
//   with all D columns as an LDS image (at most 32 KiB, dynamic LDS).
//   Phase 1 walks all n ids in chunks of 256 (L2 hits after the first workgroup) and compacts the hits
//   base <= id < base + RB into an LDS list of (token, local row) IN TOKEN ORDER: the in-wave rank is mbcnt of the
//   wave's ballot, the cross-wave offset comes from the four waves' counts through LDS (double-buffered by chunk
//   parity: one barrier per chunk).  The list holds kCap = 512 entries; whenever fewer than 256 are free, phase 2
//   drains it, so any number of hits works.
//   Phase 2: wave w takes the entries with row % 4 == w, in list order (a ballot over 64 entries, then the set
//   bits from the lowest), lanes over the float4 columns of dy[token], pure adds into the image.  A row has one
//   wave and a column one lane for the whole launch, so an element's order of summation is the token order whatever
//   the waves' progress.  Eight entries' dy loads (four above D = 256) are issued before their dependent adds.
//   Epilogue: the image, zeros included, goes to dtable with 16-byte stores (rows past V are not stored): the
//   launch writes the whole gradient, there is no memset and no accumulate mode.
#include "tde_common.h"

#include <algorithm>
#include <cstdint>

namespace tde {
namespace embed {

constexpr int kThreads = 256, kWaves = 4;
constexpr int kCap = 512;            // list entries; a chunk appends at most kThreads
constexpr int kMaxD = 512;
constexpr int kImageFloats = 8192;   // 32 KiB
constexpr int kLoads = 8;            // 16-byte dy loads in flight per lane: 8 rows, 4 where a row is two columns

// the id of token t as a row index, or -1 where it lies outside [0, V)
__device__ __forceinline__ int load_id(const void* ids, int t, int V, int is_int) {
  if (is_int) {
    const int v = static_cast<const int*>(ids)[t];
    return (unsigned)v < (unsigned)V ? v : -1;
  }
  const float f = static_cast<const float*>(ids)[t];
  return (f > -1.f && f < (float)V) ? (int)f : -1;   // truncation toward zero; NaN fails both tests
}

__global__ __launch_bounds__(kThreads) void embed_fwd_kernel(const void* __restrict__ ids,
                                                             const f32x4* __restrict__ table, f32x4* __restrict__ out,
                                                             int n, int V, int D4, int is_int) {
  const int lane = threadIdx.x & 63;
  const int tpw = D4 >= 64 ? 1 : 64 / D4;            // tokens per wave pass
  const int slot = D4 >= 64 ? 0 : lane / D4;         // the lane's token of the pass
  const int col = D4 >= 64 ? lane : lane - slot * D4;
  const int passes = (n + tpw - 1) / tpw;
  const int wave = blockIdx.x * kWaves + (threadIdx.x >> 6), nwaves = gridDim.x * kWaves;
  for (int p = wave; p < passes; p += nwaves) {
    const int t0 = p * tpw;
    int idv = -1;
    if (lane < tpw && t0 + lane < n) idv = load_id(ids, t0 + lane, V, is_int);
    const int id = __shfl(idv, slot, 64);            // slot == tpw (lanes past the last whole row) reads a -1 or
    const int t = t0 + slot;                         // a stranger's id and is masked right here
    if (slot >= tpw || t >= n) continue;
    for (int c = col; c < D4; c += 64) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (id >= 0) v = table[(size_t)id * D4 + c];
      out[(size_t)t * D4 + c] = v;
    }
  }
}

// CP = float4 columns per lane: 1 for D <= 256, 2 above
template <int CP>
__global__ __launch_bounds__(kThreads) void embed_bwd_kernel(const void* __restrict__ ids,
                                                             const f32x4* __restrict__ dy, f32x4* __restrict__ dtable,
                                                             int n, int V, int D4, int RB, int is_int) {
  constexpr int kUnroll = kLoads / CP;
  extern __shared__ f32x4 image[];                   // [RB][D4]
  __shared__ int2 list[kCap];                        // (token, local row), token order
  __shared__ int wcnt[2][kWaves];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int base = blockIdx.x * RB;
  const int rows = min(RB, V - base);                // >= 1 by the grid

  for (int i = tid; i < RB * D4; i += kThreads) image[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  // phase 2 on list[0 .. count): called by all threads between two barriers.  The wave keeps the image row it is
  // adding to in registers for as long as its entries name the same row, so a hot row's chain is one add per token,
  // not an LDS round trip; the adds and their order are the same either way.
  auto drain = [&](int count) {
    int cur = -1;
    f32x4 acc[CP];
    auto flush = [&]() {
#pragma unroll
      for (int k = 0; k < CP; ++k) {
        const int c = lane + 64 * k;
        if (cur >= 0 && c < D4) image[cur * D4 + c] = acc[k];
      }
    };
    for (int e0 = 0; e0 < count; e0 += 64) {
      int2 ent = {0, -1};
      if (e0 + lane < count) ent = list[e0 + lane];
      unsigned long long mask = __ballot(ent.y >= 0 && (ent.y & 3) == w);
      while (mask) {
        int tok[kUnroll], row[kUnroll];
        bool on[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          on[u] = mask != 0;
          const int j = on[u] ? __builtin_ctzll(mask) : 0;
          mask &= mask - 1;                          // 0 stays 0
          tok[u] = __builtin_amdgcn_readlane(ent.x, j);
          row[u] = __builtin_amdgcn_readlane(ent.y, j);
        }
        f32x4 g[kUnroll][CP];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
#pragma unroll
          for (int k = 0; k < CP; ++k) {
            const int c = lane + 64 * k;
            if (on[u] && c < D4) g[u][k] = dy[(size_t)tok[u] * D4 + c];
          }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          if (!on[u]) continue;
          if (row[u] != cur) {                       // uniform: row and cur are the wave's
            flush();
            cur = row[u];
#pragma unroll
            for (int k = 0; k < CP; ++k) {
              const int c = lane + 64 * k;
              if (c < D4) acc[k] = image[cur * D4 + c];
            }
          }
#pragma unroll
          for (int k = 0; k < CP; ++k)
            if (lane + 64 * k < D4) acc[k] = acc[k] + g[u][k];
        }
      }
    }
    flush();
  };

  int count = 0;
  const int chunks = (n + kThreads - 1) / kThreads;
  for (int ch = 0; ch < chunks; ++ch) {
    const int t = ch * kThreads + tid;
    int r = -1;
    if (t < n) {
      const int id = load_id(ids, t, V, is_int);
      if (id >= base && id < base + rows) r = id - base;
    }
    const unsigned long long hits = __ballot(r >= 0);
    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(hits >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hits, 0));
    if (lane == 0) wcnt[ch & 1][w] = __popcll(hits);
    __syncthreads();                                 // also orders the image's zeros and a drain's list reads
    int off = count, total = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const int c = wcnt[ch & 1][k];
      if (k < w) off += c;
      total += c;
    }
    if (r >= 0) list[off + rank] = int2{t, r};       // off + rank < count + 256 <= kCap
    count += total;
    if (count > kCap - kThreads) {                   // uniform: every thread holds the same count
      __syncthreads();
      drain(count);
      count = 0;                                     // the next chunk's barrier precedes its list writes
    }
  }
  __syncthreads();
  drain(count);
  __syncthreads();
  for (int i = tid; i < rows * D4; i += kThreads) dtable[(size_t)base * D4 + i] = image[i];
}

static bool geo_ok(int n, int V, int D) {
  if (n < 1 || V < 1 || V > (1 << 24) || D < 4 || D > kMaxD || D % 4) return false;
  return (long long)n * D < (1LL << 31) && (long long)V * D < (1LL << 31);
}

}  // namespace embed
}  // namespace tde

using namespace tde::embed;

// out [n, D] = table[id]; zero rows for ids outside [0, V).  ids: float32 [n], or int32 with ids_are_int
TDE_API int tde_embed32_fwd(const void* ids, const float* table, float* out, int n, int V, int D, int ids_are_int,
                            hipStream_t stream) {
  if (!geo_ok(n, V, D)) return -1;
  if (!ids || !table || !out) return -2;
  const int D4 = D / 4, tpw = D4 >= 64 ? 1 : 64 / D4;
  const int passes = (n + tpw - 1) / tpw;
  const int grid = std::min((passes + kWaves - 1) / kWaves, 8192);
  embed_fwd_kernel<<<grid, kThreads, 0, stream>>>(ids, reinterpret_cast<const f32x4*>(table),
                                                  reinterpret_cast<f32x4*>(out), n, V, D4, ids_are_int);
  TDE_LAUNCH_CHECK();
  return 0;
}

// dtable [V, D], every element written: the sum of dy [n, D] rows by id, in token order
TDE_API int tde_embed32_bwd(const void* ids, const float* dy, float* dtable, int n, int V, int D, int ids_are_int,
                            hipStream_t stream) {
  if (!geo_ok(n, V, D)) return -1;
  if (!ids || !dy || !dtable) return -2;
  const int D4 = D / 4, RB = std::min(64, kImageFloats / D);
  const int grid = (V + RB - 1) / RB;
  const size_t lds = (size_t)RB * D * sizeof(float);
  if (D4 <= 64)
    embed_bwd_kernel<1><<<grid, kThreads, lds, stream>>>(ids, reinterpret_cast<const f32x4*>(dy),
                                                         reinterpret_cast<f32x4*>(dtable), n, V, D4, RB, ids_are_int);
  else
    embed_bwd_kernel<2><<<grid, kThreads, lds, stream>>>(ids, reinterpret_cast<const f32x4*>(dy),
                                                         reinterpret_cast<f32x4*>(dtable), n, V, D4, RB, ids_are_int);
  TDE_LAUNCH_CHECK();
  return 0;
}
