// Depthwise 2-D convolution, float32 forms: forward, input gradient, weight (+ bias) gradient.
//
// A depthwise convolution contracts over KH*KW only, per channel: it has no matrix shape (the implicit
// GEMM of layers_f32.hip contracts over KH*KW*C), it is memory-bound (9-49 FMAs per output) and every
// input byte should cross HBM once.  Tensors are NHWC, the kernel is the Keras depthwise_kernel
// [KH, KW, C, dm] read in place from the f32 master: flat (tap, co) with co = c*dm + m.
//
// * One workgroup owns an output tile TH x TW of one image times a block of CBI input channels (CBO =
//   CBI*dm output channels).  It stages the input halo tile ((TH-1)*sh+KH) x ((TW-1)*sw+KW) x CBI into
//   LDS, channels innermost, 16-byte global loads when C % 4 == 0 (the V = 4 forms; V = 1 is the scalar
//   channel form for C = 1, 3, 6 ...); padding and out-of-image positions are stored as zeros, so the
//   compute loops have no bounds checks.  The block's weights are staged once.
// * Lanes run over channel quads first (conflict-free ds_read_b128 rows, coalesced global traffic along
//   C) and pixels second (a small C still fills the wave).  Each thread walks a strip of 4 outputs along
//   W per kernel row with a register window of (4-1)*sw+KW inputs: an LDS value is read once per strip,
//   not once per tap (sw = 1 and 2 are compile-time; 3 and 4 read per tap).  dm > 1 only changes which
//   LDS channel a lane reads.
// * Input gradient: stride 1 / dm 1 IS a depthwise convolution of dy with the flipped kernel and pads
//   (K-1-p), so it runs the forward kernel (weights flipped while staged).  Otherwise the gather form
//   over a staged dy tile: an input pixel visits only the taps of its stride phase, dm > 1 sums its m
//   outputs per input channel.  With y given, dy is multiplied by (y > 0) while it is staged (the
//   layer's ReLU backward); accum adds onto dx.
// * Weight gradient: the output is tiny (KH*KW*Co) and the reduction long (B*Ho*Wo): grid = channel
//   blocks x S splits of the pixel tiles.  A workgroup streams its tiles through LDS with the same halo
//   stager; a thread owns one kernel row of one channel quad (KW tap accumulators in registers, so 7x7
//   does not spill) on one of PL pixel lanes, and walks strips with the forward's register window.
//   Lanes are summed through LDS in lane order, one partial row per split is written, and a second small
//   launch sums the S rows in split order: no atomics, bitwise reproducible.
#include "tde_common.h"

#include <initializer_list>

namespace tde {
namespace dw {

struct Geo {  // NHWC input [B,H,W,C], kernel [KH,KW,C,dm], NHWC output [B,Ho,Wo,Co = C*dm]
  int B, H, W, C, Ho, Wo, Co, KH, KW, sh, sw, pt, pl;
};

static Geo geo_of(const int* p) {
  Geo g;
  g.B = p[0]; g.H = p[1]; g.W = p[2]; g.C = p[3]; g.Ho = p[4]; g.Wo = p[5]; g.Co = p[6];
  g.KH = p[7]; g.KW = p[8]; g.sh = p[9]; g.sw = p[10]; g.pt = p[11]; g.pl = p[12];
  return g;
}

constexpr int kThreads = 256;
constexpr int kStrip = 4;                 // outputs along W per thread and kernel row
constexpr int kLdsBudget = 48 * 1024;     // bytes of LDS per workgroup (three workgroups per CU)
constexpr int kMaxK = 7, kMaxStride = 4, kMaxDm = 8;
constexpr unsigned kMaxGridY = 65535;     // channel blocks (forward, input gradient) or splits ride in grid.y

template <int V> struct VecOf;
template <> struct VecOf<1> { typedef float T; };
template <> struct VecOf<4> { typedef f32x4 T; };

__device__ __forceinline__ float getc(float v, int) { return v; }
__device__ __forceinline__ float getc(const f32x4& v, int e) { return v[e]; }
__device__ __forceinline__ void setc(float& v, int, float x) { v = x; }
__device__ __forceinline__ void setc(f32x4& v, int e, float x) { v[e] = x; }

// floor(a / b) for b > 0 and any a
__host__ __device__ __forceinline__ int fdiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// Stage rows x cols pixels x cb channels of an NHWC tensor [.,H,W,C] at (b, h0, w0, c0) into
// lds[(r*cols + q)*cb + c]; out-of-image pixels and channels >= C become zeros.  With `mask`, an element is
// kept only where mask > 0 (the ReLU backward applied while staging).  cb % V == 0; V == 4 needs C % 4 == 0.
template <int V>
__device__ __forceinline__ void stage(const float* __restrict__ src, const float* __restrict__ mask, float* lds,
                                      int b, int h0, int w0, int rows, int cols, int c0, int cb, int H, int W, int C) {
  typedef typename VecOf<V>::T T;
  const int nq = cb / V, n = rows * cols * nq;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const int q = i % nq, p = i / nq, r = p / cols, cc = p - r * cols;
    const int h = h0 + r, w = w0 + cc, c = c0 + q * V;
    T v = T{};
    if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W && c < C) {
      const size_t off = (((size_t)b * H + h) * W + w) * C + c;
      v = *reinterpret_cast<const T*>(src + off);
      if (mask) {
        const T m = *reinterpret_cast<const T*>(mask + off);
#pragma unroll
        for (int e = 0; e < V; ++e) setc(v, e, getc(m, e) > 0.f ? getc(v, e) : 0.f);
      }
    }
    *reinterpret_cast<T*>(lds + (size_t)p * cb + q * V) = v;
  }
}

// wl[tap*cbo + j] = w[tap'*Co + co0 + j] (zero for co0 + j >= Co); flip: tap' = taps-1-tap
__device__ __forceinline__ void stage_w(const float* __restrict__ w, float* wl, int taps, int co0, int cbo, int Co,
                                        int flip) {
  for (int i = threadIdx.x; i < taps * cbo; i += kThreads) {
    const int j = i % cbo, tap = i / cbo, co = co0 + j;
    wl[i] = co < Co ? w[(size_t)(flip ? taps - 1 - tap : tap) * Co + co] : 0.f;
  }
}

// the V input channels an output-channel quad reads at one staged pixel: channel (oq*V + e) / dm
template <int V>
__device__ __forceinline__ typename VecOf<V>::T ldx(const float* pix, int oq, const int* ci, int dm) {
  typedef typename VecOf<V>::T T;
  if (dm == 1) return *reinterpret_cast<const T*>(pix + oq * V);
  T r = T{};
#pragma unroll
  for (int e = 0; e < V; ++e) setc(r, e, pix[ci[e]]);
  return r;
}

struct Tile {
  int TH, TW, CBI;      // output tile and input channels per workgroup
  int RH, RW;           // staged rows / columns
  size_t lds;           // bytes
};

// ---------------------------------------------------------------------------------------- forward
struct FwdP {
  const float* x;
  const float* mask;    // flipped-kernel input gradient: y of the layer (ReLU mask on the staged dy), or null
  const float* w;
  const float* bias;
  float* y;
  Geo g;
  int dm, TH, TW, CBI, IH, IW, tilesH, tilesW, relu, accum, flip;
};

template <int V, int KW, int SWS>
__global__ __launch_bounds__(kThreads) void dw_fwd_kernel(FwdP p) {
  typedef typename VecOf<V>::T T;
  extern __shared__ float4 dw_smem4[];
  float* xl = reinterpret_cast<float*>(dw_smem4);
  const Geo& g = p.g;
  const int CBI = p.CBI, CBO = CBI * p.dm, IW = p.IW;
  float* wl = xl + ((p.IH * IW * CBI + 3) & ~3);
  int t = blockIdx.x;
  const int tw = t % p.tilesW;
  t /= p.tilesW;
  const int th = t % p.tilesH, b = t / p.tilesH;
  const int c0 = blockIdx.y * CBI, co0 = c0 * p.dm, oh0 = th * p.TH, ow0 = tw * p.TW;
  stage<V>(p.x, p.mask, xl, b, oh0 * g.sh - g.pt, ow0 * g.sw - g.pl, p.IH, IW, c0, CBI, g.H, g.W, g.C);
  stage_w(p.w, wl, g.KH * KW, co0, CBO, g.Co, p.flip);
  __syncthreads();
  const int sw = SWS ? SWS : g.sw;
  const int nq = CBO / V, strips_w = p.TW / kStrip, items = p.TH * strips_w * nq;
  for (int it = threadIdx.x; it < items; it += kThreads) {
    const int oq = it % nq, s = it / nq, sx = s % strips_w, oy = s / strips_w;
    const int oh = oh0 + oy, owb = ow0 + sx * kStrip, co = co0 + oq * V;
    if (oh >= g.Ho || owb >= g.Wo || co >= g.Co) continue;
    int ci[V];
#pragma unroll
    for (int e = 0; e < V; ++e) ci[e] = (oq * V + e) / p.dm;
    T bv = T{};
    if (p.bias) {
#pragma unroll
      for (int e = 0; e < V; ++e) setc(bv, e, p.bias[co + e]);
    }
    T acc[kStrip];
#pragma unroll
    for (int o = 0; o < kStrip; ++o) acc[o] = bv;
    for (int kh = 0; kh < g.KH; ++kh) {
      const float* xr = xl + (size_t)((oy * g.sh + kh) * IW + sx * kStrip * sw) * CBI;
      const float* wr = wl + kh * KW * CBO + oq * V;
      T wv[KW];
#pragma unroll
      for (int kw = 0; kw < KW; ++kw) wv[kw] = *reinterpret_cast<const T*>(wr + kw * CBO);
      if constexpr (SWS != 0) {
        constexpr int NWIN = (kStrip - 1) * SWS + KW;
        T xin[NWIN];
#pragma unroll
        for (int j = 0; j < NWIN; ++j) xin[j] = ldx<V>(xr + j * CBI, oq, ci, p.dm);
#pragma unroll
        for (int o = 0; o < kStrip; ++o)
#pragma unroll
          for (int kw = 0; kw < KW; ++kw) acc[o] += xin[o * SWS + kw] * wv[kw];
      } else {
#pragma unroll
        for (int o = 0; o < kStrip; ++o)
#pragma unroll
          for (int kw = 0; kw < KW; ++kw) acc[o] += ldx<V>(xr + (o * sw + kw) * CBI, oq, ci, p.dm) * wv[kw];
      }
    }
#pragma unroll
    for (int o = 0; o < kStrip; ++o) {
      const int ow = owb + o;
      if (ow >= g.Wo) break;
      T r = acc[o];
      if (p.relu) {
#pragma unroll
        for (int e = 0; e < V; ++e) setc(r, e, fmaxf(getc(r, e), 0.f));
      }
      T* dst = reinterpret_cast<T*>(p.y + (((size_t)b * g.Ho + oh) * g.Wo + ow) * g.Co + co);
      if (p.accum) r += *dst;
      *dst = r;
    }
  }
}

// ---------------------------------------------------------------------------------------- input gradient (gather)
struct DgP {
  const float* dy;
  const float* mask;
  const float* w;
  float* dx;
  Geo g;
  int dm, TH, TW, CBI, DH, DW, tilesH, tilesW, accum;
};

template <int V>
__global__ __launch_bounds__(kThreads) void dw_dgrad_kernel(DgP p) {
  typedef typename VecOf<V>::T T;
  extern __shared__ float4 dw_smem4[];
  float* dl = reinterpret_cast<float*>(dw_smem4);
  const Geo& g = p.g;
  const int CBI = p.CBI, dm = p.dm, CBO = CBI * dm, DW = p.DW;
  float* wl = dl + ((p.DH * DW * CBO + 3) & ~3);
  int t = blockIdx.x;
  const int tw = t % p.tilesW;
  t /= p.tilesW;
  const int th = t % p.tilesH, b = t / p.tilesH;
  const int c0 = blockIdx.y * CBI, co0 = c0 * dm, h0 = th * p.TH, w0 = tw * p.TW;
  // first output row / column any pixel of the tile gathers from: ceil((h0 + pt - (KH-1)) / sh)
  const int oh_lo = fdiv(h0 + g.pt - (g.KH - 1) + g.sh - 1, g.sh);
  const int ow_lo = fdiv(w0 + g.pl - (g.KW - 1) + g.sw - 1, g.sw);
  stage<V>(p.dy, p.mask, dl, b, oh_lo, ow_lo, p.DH, DW, co0, CBO, g.Ho, g.Wo, g.Co);
  stage_w(p.w, wl, g.KH * g.KW, co0, CBO, g.Co, 0);
  __syncthreads();
  const int nq = CBI / V, items = p.TH * p.TW * nq;
  for (int it = threadIdx.x; it < items; it += kThreads) {
    const int cq = it % nq, pix = it / nq, px = pix % p.TW, py = pix / p.TW;
    const int h = h0 + py, w = w0 + px, c = c0 + cq * V;
    if (h >= g.H || w >= g.W || c >= g.C) continue;
    T acc = T{};
    for (int kh = (h + g.pt) % g.sh; kh < g.KH; kh += g.sh) {     // the taps of this pixel's stride phase
      const int hh = h + g.pt - kh;
      if (hh < 0) break;
      const int r = hh / g.sh - oh_lo;
      for (int kw = (w + g.pl) % g.sw; kw < g.KW; kw += g.sw) {
        const int ww = w + g.pl - kw;
        if (ww < 0) break;
        const float* dp = dl + (size_t)(r * DW + (ww / g.sw - ow_lo)) * CBO;
        const float* wp = wl + (kh * g.KW + kw) * CBO;
        if (dm == 1) {
          acc += *reinterpret_cast<const T*>(dp + cq * V) * *reinterpret_cast<const T*>(wp + cq * V);
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e) {
            const int base = (cq * V + e) * dm;
            float s = 0.f;
            for (int m = 0; m < dm; ++m) s += dp[base + m] * wp[base + m];
            setc(acc, e, getc(acc, e) + s);
          }
        }
      }
    }
    T* dst = reinterpret_cast<T*>(p.dx + (((size_t)b * g.H + h) * g.W + w) * g.C + c);
    if (p.accum) acc += *dst;
    *dst = acc;
  }
}

// ---------------------------------------------------------------------------------------- weight gradient
struct WgP {
  const float* x;
  const float* dy;
  const float* mask;
  float* part;          // [S][KH*KW*Co + Co]
  Geo g;
  int dm, TH, TW, CBI, IH, IW, tilesH, tilesW, NT, per, n_out;
};

template <int V, int KW, int SWS>
__global__ __launch_bounds__(kThreads) void dw_wgrad_kernel(WgP p) {
  typedef typename VecOf<V>::T T;
  extern __shared__ float4 dw_smem4[];
  float* xl = reinterpret_cast<float*>(dw_smem4);
  const Geo& g = p.g;
  const int CBI = p.CBI, CBO = CBI * p.dm, IW = p.IW, TW = p.TW;
  float* dl = xl + ((p.IH * IW * CBI + 3) & ~3);
  const int c0 = blockIdx.x * CBI, co0 = c0 * p.dm, split = blockIdx.y;
  const int sw = SWS ? SWS : g.sw;
  // thread = (channel quad oq, kernel row kh, pixel lane)
  const int nq = CBO / V, nrow = nq * g.KH, PL = kThreads / nrow;
  const int tid = threadIdx.x, oq = tid % nq, kh = (tid / nq) % g.KH, lane = tid / nrow;
  const bool active = lane < PL;
  int ci[V];
#pragma unroll
  for (int e = 0; e < V; ++e) ci[e] = (oq * V + e) / p.dm;
  T acc[KW];
#pragma unroll
  for (int kw = 0; kw < KW; ++kw) acc[kw] = T{};
  T db = T{};
  const int strips_w = TW / kStrip, strips = p.TH * strips_w;
  const int t_end = min(p.NT, (split + 1) * p.per);
  for (int tile = split * p.per; tile < t_end; ++tile) {
    int t = tile;
    const int tw = t % p.tilesW;
    t /= p.tilesW;
    const int th = t % p.tilesH, b = t / p.tilesH;
    const int oh0 = th * p.TH, ow0 = tw * TW;
    __syncthreads();   // the previous tile's readers are done
    stage<V>(p.x, nullptr, xl, b, oh0 * g.sh - g.pt, ow0 * g.sw - g.pl, p.IH, IW, c0, CBI, g.H, g.W, g.C);
    stage<V>(p.dy, p.mask, dl, b, oh0, ow0, p.TH, TW, co0, CBO, g.Ho, g.Wo, g.Co);
    __syncthreads();
    if (!active) continue;
    for (int s = lane; s < strips; s += PL) {
      const int sx = s % strips_w, oy = s / strips_w;
      T d[kStrip];   // zeros outside the image: those pixels add nothing
#pragma unroll
      for (int o = 0; o < kStrip; ++o)
        d[o] = *reinterpret_cast<const T*>(dl + (size_t)(oy * TW + sx * kStrip + o) * CBO + oq * V);
      const float* xr = xl + (size_t)((oy * g.sh + kh) * IW + sx * kStrip * sw) * CBI;
      if constexpr (SWS != 0) {
        constexpr int NWIN = (kStrip - 1) * SWS + KW;
        T xin[NWIN];
#pragma unroll
        for (int j = 0; j < NWIN; ++j) xin[j] = ldx<V>(xr + j * CBI, oq, ci, p.dm);
#pragma unroll
        for (int o = 0; o < kStrip; ++o)
#pragma unroll
          for (int kw = 0; kw < KW; ++kw) acc[kw] += xin[o * SWS + kw] * d[o];
      } else {
#pragma unroll
        for (int o = 0; o < kStrip; ++o)
#pragma unroll
          for (int kw = 0; kw < KW; ++kw) acc[kw] += ldx<V>(xr + (o * sw + kw) * CBI, oq, ci, p.dm) * d[o];
      }
      if (kh == 0) {
#pragma unroll
        for (int o = 0; o < kStrip; ++o) db += d[o];
      }
    }
  }
  __syncthreads();
  // lanes summed in lane order through LDS: red[((lane*nrow + kh*nq + oq)*(KW+1) + kw)*V + e], slot KW = bias
  float* red = xl;
  if (active) {
    T* r = reinterpret_cast<T*>(red + (size_t)((lane * nrow + kh * nq + oq) * (KW + 1)) * V);
#pragma unroll
    for (int kw = 0; kw < KW; ++kw) r[kw] = acc[kw];
    r[KW] = db;
  }
  __syncthreads();
  const int nw = g.KH * KW * CBO;
  float* out = p.part + (size_t)split * p.n_out;
  for (int i = tid; i < nw + CBO; i += kThreads) {
    const int j = i < nw ? i % CBO : i - nw, tap = i < nw ? i / CBO : 0;
    const int rkh = i < nw ? tap / KW : 0, rkw = i < nw ? tap % KW : KW;
    const int slot = ((rkh * nq + j / V) * (KW + 1) + rkw) * V + j % V;
    float s = 0.f;
    for (int l = 0; l < PL; ++l) s += red[(size_t)l * nrow * (KW + 1) * V + slot];
    if (co0 + j < g.Co) out[i < nw ? (size_t)tap * g.Co + co0 + j : (size_t)g.KH * KW * g.Co + co0 + j] = s;
  }
}

// dW / db = the S partial rows summed in split order
__global__ __launch_bounds__(kThreads) void dw_wgrad_reduce_kernel(const float* __restrict__ part, int S, int n_out,
                                                                   int n_w, float* dW, float* db) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_out) return;
  float s = 0.f;
  for (int k = 0; k < S; ++k) s += part[(size_t)k * n_out + i];
  if (i < n_w)
    dW[i] = s;
  else if (db)
    db[i - n_w] = s;
}

// ---------------------------------------------------------------------------------------- host side
static int roundup(int v, int m) { return (v + m - 1) / m * m; }

static bool geo_ok(const Geo& g) {
  if (g.B < 1 || g.H < 1 || g.W < 1 || g.C < 1 || g.Ho < 1 || g.Wo < 1 || g.Co < 1) return false;
  if (g.KH < 1 || g.KW < 1 || g.KH > kMaxK || g.KW > kMaxK) return false;
  if (g.sh < 1 || g.sw < 1 || g.sh > kMaxStride || g.sw > kMaxStride) return false;
  if (g.Co % g.C != 0 || g.Co / g.C > kMaxDm) return false;
  if (g.pt < 0 || g.pl < 0 || g.pt >= g.KH || g.pl >= g.KW) return false;
  // every tile index and staged-tile extent stays an int
  const long long tiles = (long long)g.B * ((g.Ho + 3) / 4 + (g.H + 3) / 4) * ((g.Wo + 3) / 4 + (g.W + 3) / 4);
  return tiles < (1ll << 31);
}

static int vec_of(const Geo& g, std::initializer_list<const void*> ptrs) {
  if (g.C % 4 != 0) return 1;
  for (const void* q : ptrs)
    if (q && ((uintptr_t)q & 15)) return 1;
  return 4;
}

static int chan_block(int C, int V, int dm) {
  int cbi = V == 4 ? (roundup(C, 4) < 32 ? roundup(C, 4) : 32) : (C < 16 ? C : 16);
  while (cbi * dm > 64 && cbi > V) cbi = roundup(cbi / 2, V);
  return cbi;
}

// kind 0: forward (halo from an output tile, weights), 1: gather input gradient (dy tile, weights),
// 2: weight gradient (halo + dy tile; also holds the lane reduction; fixed 8 x 8 tiles, its lanes are
// filled by pixel lanes).  Kinds 0 and 1 widen the tile until the workgroup has kThreads items (small
// channel blocks), and every kind shrinks it until the staged tiles fit the LDS budget.
static Tile pick_tile(const Geo& g, int V, int dm, int kind) {
  Tile t;
  t.CBI = chan_block(g.C, V, dm);
  // weight gradient: a thread is one (channel quad, kernel row) pair, and in the scalar form -- which an
  // unaligned operand selects for any C, on these same tiles -- one (channel, kernel row) pair: CBI*dm*KH of
  // them must fit the workgroup whichever form runs (V*dm*KH <= 4*8*7 = 224 always does)
  if (kind == 2)
    while (t.CBI * dm * g.KH > kThreads && t.CBI > V) t.CBI = roundup(t.CBI / 2, V);
  const int oh = kind == 1 ? g.H : g.Ho, ow = kind == 1 ? g.W : g.Wo;   // extents of the tiled tensor
  t.TH = 8;
  t.TW = 8;
  while (t.TH > 1 && t.TH / 2 >= oh) t.TH /= 2;
  if (ow <= 4) t.TW = 4;
  if (kind != 2) {
    const int nq = t.CBI * (kind == 0 ? dm : 1) / V;
    auto items = [&] { return t.TH * t.TW / (kind == 0 ? kStrip : 1) * nq; };
    while (items() < kThreads) {
      if (t.TW < 32 && t.TW < ow && t.TW <= t.TH) t.TW *= 2;
      else if (t.TH < 32 && t.TH < oh) t.TH *= 2;
      else if (t.TW < 32 && t.TW < ow) t.TW *= 2;
      else break;
    }
  }
  for (;;) {
    const int cbo = t.CBI * dm;
    size_t fl;
    if (kind == 1) {
      t.RH = (t.TH + g.KH - 2) / g.sh + 1;
      t.RW = (t.TW + g.KW - 2) / g.sw + 1;
      fl = (size_t)roundup(t.RH * t.RW * cbo, 4) + (size_t)g.KH * g.KW * cbo;
    } else {
      t.RH = (t.TH - 1) * g.sh + g.KH;
      t.RW = (t.TW - 1) * g.sw + g.KW;
      fl = (size_t)roundup(t.RH * t.RW * t.CBI, 4);
      if (kind == 0) fl += (size_t)g.KH * g.KW * cbo;
      if (kind == 2) {
        fl += (size_t)t.TH * t.TW * cbo;
        const size_t red = (size_t)kThreads * (g.KW + 1) * V;
        if (fl < red) fl = red;
      }
    }
    t.lds = fl * sizeof(float);
    if (t.lds <= (size_t)kLdsBudget) break;
    if (t.TH > 1) t.TH /= 2;
    else if (t.TW > kStrip) t.TW /= 2;
    else if (t.CBI > V) t.CBI = roundup(t.CBI / 2, V);
    else break;
  }
  return t;
}

// pixel-tile splits of the weight gradient: fill the chip (2 workgroups per CU over all channel blocks), at
// least two tiles per split so that the staging amortises the lane reduction
static void wgrad_split(const Geo& g, const Tile& t, int* S, int* per, int* NT) {
  const int ncb = (g.C + t.CBI - 1) / t.CBI;
  const long long nt = (long long)g.B * ((g.Ho + t.TH - 1) / t.TH) * ((g.Wo + t.TW - 1) / t.TW);
  long long s0 = (512 + ncb - 1) / ncb;
  if (s0 > (nt + 1) / 2) s0 = (nt + 1) / 2;
  if (s0 < 1) s0 = 1;
  *per = (int)((nt + s0 - 1) / s0);
  *S = (int)((nt + *per - 1) / *per);
  *NT = (int)nt;
}

#define DW_KW_CASES(LAUNCH, V, SWS)  \
  switch (g.KW) {                    \
    case 1: LAUNCH(V, 1, SWS); break; \
    case 2: LAUNCH(V, 2, SWS); break; \
    case 3: LAUNCH(V, 3, SWS); break; \
    case 4: LAUNCH(V, 4, SWS); break; \
    case 5: LAUNCH(V, 5, SWS); break; \
    case 6: LAUNCH(V, 6, SWS); break; \
    default: LAUNCH(V, 7, SWS); break; \
  }
#define DW_DISPATCH(LAUNCH)                                      \
  do {                                                           \
    const int sws__ = g.sw <= 2 ? g.sw : 0;                      \
    if (V == 4) {                                                \
      if (sws__ == 1) { DW_KW_CASES(LAUNCH, 4, 1) }              \
      else if (sws__ == 2) { DW_KW_CASES(LAUNCH, 4, 2) }         \
      else { DW_KW_CASES(LAUNCH, 4, 0) }                         \
    } else {                                                     \
      if (sws__ == 1) { DW_KW_CASES(LAUNCH, 1, 1) }              \
      else if (sws__ == 2) { DW_KW_CASES(LAUNCH, 1, 2) }         \
      else { DW_KW_CASES(LAUNCH, 1, 0) }                         \
    }                                                            \
  } while (0)

static int launch_fwd(const float* x, const float* mask, const float* w, const float* bias, int relu, float* y,
                      const Geo& g, int accum, int flip, hipStream_t stream) {
  const int dm = g.Co / g.C, V = vec_of(g, {x, mask, y});
  const Tile t = pick_tile(g, V, dm, 0);
  if (t.lds > (size_t)kLdsBudget) return -3;
  FwdP p;
  p.x = x; p.mask = mask; p.w = w; p.bias = bias; p.y = y; p.g = g; p.dm = dm;
  p.TH = t.TH; p.TW = t.TW; p.CBI = t.CBI; p.IH = t.RH; p.IW = t.RW;
  p.tilesH = (g.Ho + t.TH - 1) / t.TH;
  p.tilesW = (g.Wo + t.TW - 1) / t.TW;
  p.relu = relu; p.accum = accum; p.flip = flip;
  const dim3 grid((unsigned)(g.B * p.tilesH * p.tilesW), (unsigned)((g.C + t.CBI - 1) / t.CBI));
  if (grid.y > kMaxGridY) return -4;
#define DW_FWD(V_, KW_, SWS_) dw_fwd_kernel<V_, KW_, SWS_><<<grid, kThreads, t.lds, stream>>>(p)
  DW_DISPATCH(DW_FWD);
#undef DW_FWD
  TDE_LAUNCH_CHECK();
  return 0;
}

}  // namespace dw
}  // namespace tde

using namespace tde::dw;

// y = act(bias + depthwise_conv(x, w)); geo = {B,H,W,C,Ho,Wo,Co,KH,KW,sh,sw,pt,pl}, Co = C*dm.
TDE_API int tde_dwconv32_fwd(const float* x, const float* w, const float* bias, int relu, float* y, const int* geo,
                             hipStream_t stream) {
  const Geo g = geo_of(geo);
  if (!x || !w || !y || !geo_ok(g)) return -1;
  return launch_fwd(x, nullptr, w, bias, relu, y, g, 0, 0, stream);
}

// dx (+)= input gradient of dy * (y > 0 if y).
TDE_API int tde_dwconv32_dgrad(const float* dy, const float* y, const float* w, float* dx, int accum, const int* geo,
                               hipStream_t stream) {
  const Geo g = geo_of(geo);
  if (!dy || !w || !dx || !geo_ok(g)) return -1;
  const int dm = g.Co / g.C;
  if (g.sh == 1 && g.sw == 1 && dm == 1) {
    // a depthwise convolution of dy [B,Ho,Wo,C] with the flipped kernel, pads (K-1-p), onto dx [B,H,W,C]
    Geo f = g;
    f.H = g.Ho; f.W = g.Wo; f.Ho = g.H; f.Wo = g.W;
    f.pt = g.KH - 1 - g.pt;
    f.pl = g.KW - 1 - g.pl;
    return launch_fwd(dy, y, w, nullptr, 0, dx, f, accum, 1, stream);
  }
  const int V = vec_of(g, {dy, y, dx});
  const Tile t = pick_tile(g, V, dm, 1);
  if (t.lds > (size_t)kLdsBudget) return -3;
  DgP p;
  p.dy = dy; p.mask = y; p.w = w; p.dx = dx; p.g = g; p.dm = dm;
  p.TH = t.TH; p.TW = t.TW; p.CBI = t.CBI; p.DH = t.RH; p.DW = t.RW;
  p.tilesH = (g.H + t.TH - 1) / t.TH;
  p.tilesW = (g.W + t.TW - 1) / t.TW;
  p.accum = accum;
  const dim3 grid((unsigned)(g.B * p.tilesH * p.tilesW), (unsigned)((g.C + t.CBI - 1) / t.CBI));
  if (grid.y > kMaxGridY) return -4;
  if (V == 4)
    dw_dgrad_kernel<4><<<grid, kThreads, t.lds, stream>>>(p);
  else
    dw_dgrad_kernel<1><<<grid, kThreads, t.lds, stream>>>(p);
  TDE_LAUNCH_CHECK();
  return 0;
}

// Number of pixel splits of the weight gradient at this geometry (part holds splits * (KH*KW*Co + Co) floats).
// The vector form is assumed for C % 4 == 0: an unaligned operand takes the scalar form with the SAME tiles.
TDE_API int tde_dwconv32_splits(const int* geo) {
  const Geo g = geo_of(geo);
  if (!geo_ok(g)) return -1;
  const int dm = g.Co / g.C;
  const Tile t = pick_tile(g, g.C % 4 == 0 ? 4 : 1, dm, 2);
  int S, per, NT;
  wgrad_split(g, t, &S, &per, &NT);
  return S;
}

// dW[tap, co] = sum x . dy * (y > 0 if y), db[co] = sum of that dy (if db); part: tde_dwconv32_splits rows.
TDE_API int tde_dwconv32_wgrad(const float* x, const float* dy, const float* y, float* dW, float* db, float* part,
                               const int* geo, hipStream_t stream) {
  const Geo g = geo_of(geo);
  if (!x || !dy || !dW || !part || !geo_ok(g)) return -1;
  const int dm = g.Co / g.C;
  // tiles (and so the split count) follow C % 4 alone; unaligned operands run them on the scalar form
  const Tile t = pick_tile(g, g.C % 4 == 0 ? 4 : 1, dm, 2);
  const int V = vec_of(g, {x, dy, y});
  if (t.lds > (size_t)kLdsBudget) return -3;
  WgP p;
  p.x = x; p.dy = dy; p.mask = y; p.part = part; p.g = g; p.dm = dm;
  p.TH = t.TH; p.TW = t.TW; p.CBI = t.CBI; p.IH = t.RH; p.IW = t.RW;
  p.tilesH = (g.Ho + t.TH - 1) / t.TH;
  p.tilesW = (g.Wo + t.TW - 1) / t.TW;
  int S;
  wgrad_split(g, t, &S, &p.per, &p.NT);
  p.n_out = g.KH * g.KW * g.Co + g.Co;
  if ((t.CBI * dm / V) * g.KH > kThreads) return -3;
  const dim3 grid((unsigned)((g.C + t.CBI - 1) / t.CBI), (unsigned)S);
  if (grid.y > kMaxGridY) return -4;
#define DW_WG(V_, KW_, SWS_) dw_wgrad_kernel<V_, KW_, SWS_><<<grid, kThreads, t.lds, stream>>>(p)
  DW_DISPATCH(DW_WG);
#undef DW_WG
  TDE_LAUNCH_CHECK();
  dw_wgrad_reduce_kernel<<<(p.n_out + kThreads - 1) / kThreads, kThreads, 0, stream>>>(part, S, p.n_out,
                                                                                        g.KH * g.KW * g.Co, dW, db);
  TDE_LAUNCH_CHECK();
  return 0;
}
