// Fused NHWC BatchNorm kernels for gfx950 — the hot elementwise path of the
// ResNet benchmark (BASELINE headline). Replaces MIOpen's unfused
// BatchNorm + separate residual-add + ReLU (+ fp32 autocast conversions)
// with bf16-native fused kernels:
//
//   fwd:  reduce(sum,sumsq) -> finalize(scale/shift, running stats)
//         -> apply: y = relu(x*scale + shift [+ residual])
//            [+ mask: y > 0 packed to 1 bit per element, for backward]
//   bwd:  reduce(sum_dz, sum_dz*xhat; dz = relu-masked dy, the mask read
//                from y or from the packed bits)
//         -> finalize(k1..k3, dweight, dbias)
//         -> apply: dx = k1*(dz - k2 - xhat*k3)  [+ dres = dz]
//
// Layout: channels_last => x is M x C row-major (M = N*H*W), C contiguous.
// Each thread owns a FIXED 8-channel group (bf16x8 = 16 B loads), so
// per-channel coefficients live in registers, not LDS lookups. Reductions:
// in-register accumulate over rows -> LDS cross-row reduce -> one fp32
// atomicAdd per channel per block. fp32 math throughout.
#include "common.h"

#define BN_VEC 8  // channels per thread (8 x bf16 = 16B; C must be mult of 8)
// Rows whose loads a thread issues before it consumes any of them, in the
// streaming reduces (BN_RED_U) and in the finalize kernels (BN_FIN_U). The
// reduce grids are small (at most BN_GM_MAX blocks per channel column), so
// one load per trip leaves HBM latency uncovered. The rows are still added
// one after the other in their old order: the sums do not change by a bit.
#define BN_RED_U 4
#define BN_FIN_U 8
// Rows in flight in the streaming apply kernels, per family: forward
// (bn_fwd_apply_kernel, bn_fwd_apply_add_bn_kernel), backward
// (bn_bwd_apply_kernel but its pool variant) and the two-branch backward
// (bn_bwd_apply2_kernel). These kernels are elementwise: the value only
// moves time. 1 leaves the one-row loop alone.
#ifndef BN_APPLY_FWD_U
#define BN_APPLY_FWD_U 2
#endif
#ifndef BN_APPLY_BWD_U
#define BN_APPLY_BWD_U 2
#endif
#ifndef BN_APPLY2_U
#define BN_APPLY2_U 2
#endif
// how the backward kernels get the ReLU mask: not at all, from the sign of
// the stored y, or from the bit-packed mask the forward apply kernel wrote
#define BN_RELU_NONE 0
#define BN_RELU_Y 1
#define BN_RELU_MASK 2

// vector load/store helpers: 8 channels
__device__ __forceinline__ void load8(const __hip_bfloat16* p, float* v) {
  // 16B load
  const __hip_bfloat162* p2 = reinterpret_cast<const __hip_bfloat162*>(p);
  float2 a = __bfloat1622float2(p2[0]);
  float2 b = __bfloat1622float2(p2[1]);
  float2 c = __bfloat1622float2(p2[2]);
  float2 d = __bfloat1622float2(p2[3]);
  v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
  v[4] = c.x; v[5] = c.y; v[6] = d.x; v[7] = d.y;
}
__device__ __forceinline__ void store8(__hip_bfloat16* p, const float* v) {
  __hip_bfloat162* p2 = reinterpret_cast<__hip_bfloat162*>(p);
  p2[0] = __float22bfloat162_rn({v[0], v[1]});
  p2[1] = __float22bfloat162_rn({v[2], v[3]});
  p2[2] = __float22bfloat162_rn({v[4], v[5]});
  p2[3] = __float22bfloat162_rn({v[6], v[7]});
}
// store8 plus the packed ReLU mask of what was stored: bit k is set iff the
// value now in p[k] (after rounding to T) is > 0
__device__ __forceinline__ unsigned store8_mask(__hip_bfloat16* p,
                                                const float* v) {
  __hip_bfloat162* p2 = reinterpret_cast<__hip_bfloat162*>(p);
  unsigned bits = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    __hip_bfloat162 h = __float22bfloat162_rn({v[2 * j], v[2 * j + 1]});
    p2[j] = h;
    float2 f = __bfloat1622float2(h);
    bits |= (f.x > 0.f ? 1u : 0u) << (2 * j);
    bits |= (f.y > 0.f ? 1u : 0u) << (2 * j + 1);
  }
  return bits;
}
__device__ __forceinline__ void load8(const float* p, float* v) {
  float4 a = *reinterpret_cast<const float4*>(p);
  float4 b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void store8(float* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ unsigned store8_mask(float* p, const float* v) {
  store8(p, v);
  unsigned bits = 0;
#pragma unroll
  for (int k = 0; k < BN_VEC; ++k) bits |= (v[k] > 0.f ? 1u : 0u) << k;
  return bits;
}
// The same 8 channels as they lie in memory (4 registers for bf16), so that
// the rows an unrolled loop holds in flight stay cheap until they are used.
template <typename T> struct Raw8;
template <> struct Raw8<__hip_bfloat16> { uint4 a; };
template <> struct Raw8<float> { float4 a, b; };
__device__ __forceinline__ Raw8<__hip_bfloat16> load8raw(
    const __hip_bfloat16* p) {
  return {*reinterpret_cast<const uint4*>(p)};
}
__device__ __forceinline__ Raw8<float> load8raw(const float* p) {
  return {*reinterpret_cast<const float4*>(p),
          *reinterpret_cast<const float4*>(p + 4)};
}
// bf16 -> fp32 is exact: the 16 bits become the high half of the word
__device__ __forceinline__ void unpack8(const Raw8<__hip_bfloat16>& r,
                                        float* v) {
  const unsigned w[4] = {r.a.x, r.a.y, r.a.z, r.a.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[2 * j] = __uint_as_float(w[j] << 16);
    v[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
  }
}
__device__ __forceinline__ void unpack8(const Raw8<float>& r, float* v) {
  v[0] = r.a.x; v[1] = r.a.y; v[2] = r.a.z; v[3] = r.a.w;
  v[4] = r.b.x; v[5] = r.b.y; v[6] = r.b.z; v[7] = r.b.w;
}
// Loads through a const __restrict__ kernel argument are tied to nothing but
// their address and their use, so instruction selection may sink them below
// a sched_barrier to where they are consumed; in the backward apply kernels
// and in some forward instantiations it does. An empty asm that takes the registers
// of a row makes the row opaque at that point: its loads are issued (and
// waited for) above it, every use stays below it.
typedef unsigned bn_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void pin8(Raw8<__hip_bfloat16>& r) {
  bn_u32x4 v = {r.a.x, r.a.y, r.a.z, r.a.w};
  asm volatile("" : "+v"(v));
  r.a = make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void pin8(Raw8<float>& r) {
  bn_u32x4 a = {__float_as_uint(r.a.x), __float_as_uint(r.a.y),
                __float_as_uint(r.a.z), __float_as_uint(r.a.w)};
  bn_u32x4 b = {__float_as_uint(r.b.x), __float_as_uint(r.b.y),
                __float_as_uint(r.b.z), __float_as_uint(r.b.w)};
  asm volatile("" : "+v"(a), "+v"(b));
  r.a = make_float4(__uint_as_float(a.x), __uint_as_float(a.y),
                    __uint_as_float(a.z), __uint_as_float(a.w));
  r.b = make_float4(__uint_as_float(b.x), __uint_as_float(b.y),
                    __uint_as_float(b.z), __uint_as_float(b.w));
}
__device__ __forceinline__ void pin8(unsigned& bits) {
  asm volatile("" : "+v"(bits));
}
// dz = dy where the mask bit is set, else 0
__device__ __forceinline__ void apply_mask8(unsigned bits, float* dv) {
#pragma unroll
  for (int k = 0; k < BN_VEC; ++k) dv[k] = (bits >> k) & 1u ? dv[k] : 0.f;
}

// v as it reads back after a store to T
__device__ __forceinline__ float round_to(float v, const __hip_bfloat16*) {
  return __bfloat162float(__float2bfloat16(v));
}
__device__ __forceinline__ float round_to(float v, const float*) { return v; }

// ------------------------------------------------- 3x3 / stride 2 / pad 1 pool
// The stem's bn -> relu -> maxpool keeps no full-resolution y. The forward
// pool-apply kernel writes the pooled y and, per pooled pixel and 8 channels,
// one argmax word: nibble k holds the window position kh*3+kw (0..8) of the
// first maximum of channel c0+k (row-major window order, strict >, compared
// after rounding to T), or BN_POOL_NONE where the pooled value is not > 0, so
// the ReLU mask is folded in. Backward (BN_RELU_POOL) gathers dz of an input
// pixel from the 1, 2 or 4 windows that cover it.
#define BN_RELU_POOL 3
#define BN_POOL_NONE 15u
#define BN_POOL_NEVER 14u  // a code no nibble holds: a window that is not there
struct BNPool {
  const unsigned* amax;  // [N*Ho*Wo, C/8]
  int H, W, Ho, Wo;
};
// what one input pixel needs from the pooled side: dy and the argmax word of
// four windows in ascending (ho, wo), and the window position this pixel has
// in each. Windows that do not exist are loaded from the first one's address
// under a code that matches nothing, so all loads are unconditional and can
// be issued ahead of their use.
template <typename T>
struct PoolTaps {
  Raw8<T> d[4];
  unsigned a[4];
  unsigned codes;  // byte j: the position of the pixel in window j
};
template <typename T>
__device__ __forceinline__ void pool_issue(const T* __restrict__ dy,
                                           const BNPool& p, long m, int C,
                                           int c0, PoolTaps<T>& t) {
  // N*H*W and the pooled tensor's element count are below 2^31 (checked by
  // the host): 32-bit divisions, and one 32-bit offset per window, which
  // addresses dy and, divided by 8, the argmax word
  const unsigned mm = (unsigned)m;
  const unsigned q = mm / (unsigned)p.W;
  const int w = (int)(mm - q * (unsigned)p.W);
  const unsigned n = q / (unsigned)p.H;
  const int h = (int)(q - n * (unsigned)p.H);
  // window ho covers rows 2ho-1..2ho+1: an even h lies in window h/2 alone
  // (kh = 1), an odd h in (h-1)/2 (kh = 2) and, if it exists, (h+1)/2 (kh = 0)
  const int ho = h >> 1, wo = w >> 1;
  const bool hb = (h & 1) && ho + 1 < p.Ho;
  const bool wb = (w & 1) && wo + 1 < p.Wo;
  const unsigned kh = 1 + (h & 1), kw = 1 + (w & 1);
  const unsigned o0 = ((n * p.Ho + ho) * p.Wo + wo) * C + c0;
  const unsigned dh = hb ? p.Wo * C : 0, dw = wb ? C : 0;
  const unsigned o[4] = {o0, o0 + dw, o0 + dh, o0 + dh + dw};
  t.codes = (kh * 3 + kw) | (wb ? kh * 3 : BN_POOL_NEVER) << 8 |
            (hb ? kw : BN_POOL_NEVER) << 16 |
            (hb && wb ? 0u : BN_POOL_NEVER) << 24;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    t.d[j] = load8raw(dy + o[j]);
    t.a[j] = p.amax[o[j] / BN_VEC];
  }
}
// dz = the pooled dy of the windows whose nibble names this pixel, added in
// fp32 in ascending (ho, wo) and rounded once to T
template <typename T>
__device__ __forceinline__ void pool_dz(const PoolTaps<T>& t, float* dv) {
  float acc[BN_VEC] = {0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float d[BN_VEC];
    unpack8(t.d[j], d);
    const unsigned e = t.a[j] ^ (((t.codes >> (8 * j)) & 15u) * 0x11111111u);
#pragma unroll
    for (int k = 0; k < BN_VEC; ++k)
      acc[k] += ((e >> (4 * k)) & 15u) == 0u ? d[k] : 0.f;
  }
#pragma unroll
  for (int k = 0; k < BN_VEC; ++k) dv[k] = round_to(acc[k], (const T*)nullptr);
}

// ---------------------------------------------------------------- fwd reduce
// Two-stage, atomic-free (deterministic): each block writes one partial row
// partial[blockIdx.x][c]; the finalize kernel sums the gridM rows. (A global
// fp32 atomicAdd design serialized ~gridM-way per channel address — ~200 us
// on small tensors.)
template <typename T>
__global__ void __launch_bounds__(BLOCK_THREADS)
bn_fwd_reduce_kernel(const T* __restrict__ x, float* __restrict__ partial_sum,
                     float* __restrict__ partial_sq, long M, int C) {
  // fmaf spelled out, contraction off: left to the compiler, whether
  // q += v*v becomes one fma or a mul and an add depends on the code around
  // it, and the sums must not depend on how the loop is unrolled
#pragma clang fp contract(off)
  int tx_count = min(C / BN_VEC, (int)blockDim.x);
  int tx = threadIdx.x % tx_count;
  int ty = threadIdx.x / tx_count;
  int rows_per_blk = blockDim.x / tx_count;
  int c0 = (blockIdx.y * tx_count + tx) * BN_VEC;
  if (c0 >= C) return;
  float s[BN_VEC] = {0}, q[BN_VEC] = {0};
  const long stride = (long)gridDim.x * rows_per_blk;
  long m = (long)blockIdx.x * rows_per_blk + ty;
  for (; m + (BN_RED_U - 1) * stride < M; m += BN_RED_U * stride) {
    Raw8<T> rx[BN_RED_U];
#pragma unroll
    for (int u = 0; u < BN_RED_U; ++u)
      rx[u] = load8raw(x + (m + u * stride) * C + c0);
    // every load of the trip is issued before the first row is consumed
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < BN_RED_U; ++u) {
      float v[BN_VEC];
      unpack8(rx[u], v);
#pragma unroll
      for (int k = 0; k < BN_VEC; ++k) {
        s[k] += v[k];
        q[k] = fmaf(v[k], v[k], q[k]);
      }
    }
  }
  for (; m < M; m += stride) {
    float v[BN_VEC];
    load8(x + m * C + c0, v);
#pragma unroll
    for (int k = 0; k < BN_VEC; ++k) { s[k] += v[k]; q[k] = fmaf(v[k], v[k], q[k]); }
  }
  __shared__ float ls[BLOCK_THREADS * BN_VEC];
  __shared__ float lq[BLOCK_THREADS * BN_VEC];
#pragma unroll
  for (int k = 0; k < BN_VEC; ++k) {
    ls[threadIdx.x * BN_VEC + k] = s[k];
    lq[threadIdx.x * BN_VEC + k] = q[k];
  }
  __syncthreads();
  if (ty == 0) {
    for (int r = 1; r < rows_per_blk; ++r) {
      int o = (r * tx_count + tx) * BN_VEC;
#pragma unroll
      for (int k = 0; k < BN_VEC; ++k) { s[k] += ls[o + k]; q[k] += lq[o + k]; }
    }
    store8(partial_sum + (long)blockIdx.x * C + c0, s);
    store8(partial_sq + (long)blockIdx.x * C + c0, q);
  }
}

// ------------------------------------------------------------ fwd finalize
// scale = w*rstd; shift = b - mean*scale; running stats updated in place.
// block = 64 channels x 4 row-lanes: lanes split the grid_m partial rows so
// small-C layers still read the partial matrix with thousands of threads.
#define FIN_CH 64
#define FIN_LANES 4
// One lane's share of the partial rows (ty, ty + 4, ...) of channel c, summed
// in that order. A rolled loop left the loads nearly serial, one L2 /
// Infinity Cache latency per row; here BN_FIN_U rows are in flight at once.
__device__ __forceinline__ void bn_fin_lane_sum(const float* __restrict__ pa,
                                                const float* __restrict__ pb,
                                                int grid_m, int ty, int C,
                                                int c, float& a, float& b) {
  int r = ty;
  for (; r + (BN_FIN_U - 1) * FIN_LANES < grid_m; r += BN_FIN_U * FIN_LANES) {
    float va[BN_FIN_U], vb[BN_FIN_U];
#pragma unroll
    for (int u = 0; u < BN_FIN_U; ++u) {
      va[u] = pa[(long)(r + u * FIN_LANES) * C + c];
      vb[u] = pb[(long)(r + u * FIN_LANES) * C + c];
    }
#pragma unroll
    for (int u = 0; u < BN_FIN_U; ++u) { a += va[u]; b += vb[u]; }
  }
  for (; r < grid_m; r += FIN_LANES) {
    a += pa[(long)r * C + c];
    b += pb[(long)r * C + c];
  }
}
__global__ void bn_fwd_finalize_kernel(const float* __restrict__ partial_sum,
                                       const float* __restrict__ partial_sq,
                                       int grid_m,
                                       const float* __restrict__ weight,
                                       const float* __restrict__ bias,
                                       float* __restrict__ running_mean,
                                       float* __restrict__ running_var,
                                       float* __restrict__ save_mean,
                                       float* __restrict__ save_rstd,
                                       float* __restrict__ scale,
                                       float* __restrict__ shift, long M,
                                       int C, float eps, float momentum) {
  int tx = threadIdx.x % FIN_CH;
  int ty = threadIdx.x / FIN_CH;
  int c = blockIdx.x * FIN_CH + tx;
  if (c >= C) return;
  float s = 0.f, q = 0.f;
  bn_fin_lane_sum(partial_sum, partial_sq, grid_m, ty, C, c, s, q);
  __shared__ float ls[FIN_LANES * FIN_CH], lq[FIN_LANES * FIN_CH];
  ls[ty * FIN_CH + tx] = s;
  lq[ty * FIN_CH + tx] = q;
  __syncthreads();
  if (ty != 0) return;
#pragma unroll
  for (int r = 1; r < FIN_LANES; ++r) {
    s += ls[r * FIN_CH + tx];
    q += lq[r * FIN_CH + tx];
  }
  float mean = s / (float)M;
  float var = fmaxf(q / (float)M - mean * mean, 0.f);
  float rstd = rsqrtf(var + eps);
  float sc = weight[c] * rstd;
  save_mean[c] = mean;
  save_rstd[c] = rstd;
  scale[c] = sc;
  shift[c] = bias[c] - mean * sc;
  if (momentum > 0.f) {
    float unbiased = M > 1 ? var * (float)M / (float)(M - 1) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
  }
}

// ------------------------------------------------------------- fwd apply
// MASK (with RELU): also write the ReLU mask of the stored y, one bit per
// element: mask is [M, C/8] uint8 row-major, bit k of byte (m, c0/8) is set
// iff y[m, c0+k] > 0. A thread owns 8 channels, so it writes one byte per row.
//
// The streaming apply kernels (this one, bn_fwd_apply_add_bn_kernel,
// bn_bwd_apply_kernel, bn_bwd_apply2_kernel) share one loop shape: per trip a
// thread issues the raw loads of every stream for U rows ahead of a
// sched_barrier, then computes and stores the U rows; a one-row loop takes
// what is left. With one row per trip the loop waited for its loads and, as
// vmcnt counts stores too, for the previous row's store, with nothing in
// flight while it computed. The host sizes the grid so that the rows of a
// thread are a multiple of U wherever M allows (bn_apply_gm in ext.hip).
// The arithmetic is spelled as the one-row loops compiled it (x*scale+shift
// contracted to one fma), with contraction off, so that no unrolling moves a
// bit: tests/test_bn_pool_gpu.py and tests/test_bn_add_bn_gpu.py compare this
// kernel with the pool and joint-tail kernels, which spell fmaf as well.
template <typename T, bool RELU, bool ADD, bool MASK>
__device__ __forceinline__ void bn_fwd_apply_row(
    const Raw8<T>& rx, const Raw8<T>& rr, const float* sc, const float* sh,
    T* __restrict__ y, unsigned char* __restrict__ mask, long m, int C,
    int c0) {
#pragma clang fp contract(off)
  float v[BN_VEC];
  unpack8(rx, v);
#pragma unroll
  for (int k = 0; k < BN_VEC; ++k) v[k] = fmaf(v[k], sc[k], sh[k]);
  if (ADD) {
    float r[BN_VEC];
    unpack8(rr, r);
#pragma unroll
    for (int k = 0; k < BN_VEC; ++k) v[k] += r[k];
  }
  if (RELU) {
#pragma unroll
    for (int k = 0; k < BN_VEC; ++k) v[k] = fmaxf(v[k], 0.f);
  }
  if (MASK)
    mask[m * (C / BN_VEC) + c0 / BN_VEC] =
        (unsigned char)store8_mask(y + m * C + c0, v);
  else
    store8(y + m * C + c0, v);
}

template <typename T, bool RELU, bool ADD, bool MASK>
__global__ void __launch_bounds__(BLOCK_THREADS)
bn_fwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ res,
                    T* __restrict__ y, unsigned char* __restrict__ mask,
                    const float* __restrict__ scale,
                    const float* __restrict__ shift, long M, int C) {
  constexpr int U = BN_APPLY_FWD_U;
  int tx_count = min(C / BN_VEC, (int)blockDim.x);
  int tx = threadIdx.x % tx_count;
  int ty = threadIdx.x / tx_count;
  int rows_per_blk = blockDim.x / tx_count;
  int c0 = (blockIdx.y * tx_count + tx) * BN_VEC;
  if (c0 >= C) return;
  float sc[BN_VEC], sh[BN_VEC];
  load8(scale + c0, sc);
  load8(shift + c0, sh);
  const long stride = (long)gridDim.x * rows_per_blk;
  long m = (long)blockIdx.x * rows_per_blk + ty;
  if (U > 1) {
    for (; m + (U - 1) * stride < M; m += U * stride) {
      Raw8<T> rx[U], rr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        rx[u] = load8raw(x + (m + u * stride) * C + c0);
        if (ADD) rr[u] = load8raw(res + (m + u * stride) * C + c0);
      }
      // every load of the trip is issued before the first row is consumed
#pragma unroll
      for (int u = 0; u < U; ++u) {
        pin8(rx[u]);
        if (ADD) pin8(rr[u]);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        bn_fwd_apply_row<T, RELU, ADD, MASK>(rx[u], rr[u], sc, sh, y, mask,
                                             m + u * stride, C, c0);
        // one row unpacked at a time: interleaved, the U rows' fp32 values
        // cost more registers than the rows still packed
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  for (; m < M; m += stride) {
    Raw8<T> rx = load8raw(x + m * C + c0), rr;
    if (ADD) rr = load8raw(res + m * C + c0);
    bn_fwd_apply_row<T, RELU, ADD, MASK>(rx, rr, sc, sh, y, mask, m, C, c0);
  }
}

// ---------------------------------------------------- fwd apply + max-pool
// A thread owns 8 channels of one pooled pixel (mo = (n*Ho + ho)*Wo + wo). It
// forms relu(x*scale+shift) rounded to T, the values bn_fwd_apply_kernel
// stores, at the window's nine positions and keeps the first maximum.
// Positions outside the image are loaded from the nearest pixel inside (the
// centre always is) and skipped, so the nine loads are unconditional.
// x*scale+shift is spelled fmaf here and in bn_fwd_apply_add_bn_kernel:
// bn_fwd_apply_kernel writes v*sc+sh and the compiler contracts it to one
// fused multiply-add (v_pk_fma_f32). The pooled y and the joint tail are
// bit-equal to the split path only while that kernel stays contracted;
// tests/test_bn_pool_gpu.py and tests/test_bn_add_bn_gpu.py fail otherwise.
template <typename T>
__global__ void bn_fwd_pool_apply_kernel(const T* __restrict__ x,
                                         T* __restrict__ y,
                                         unsigned* __restrict__ amax,
                                         const float* __restrict__ scale,
                                         const float* __restrict__ shift,
                                         BNPool p, long Mo, int C) {
  int tx_count = min(C / BN_VEC, (int)blockDim.x);
  int tx = threadIdx.x % tx_count;
  int ty = threadIdx.x / tx_count;
  int rows_per_blk = blockDim.x / tx_count;
  int c0 = (blockIdx.y * tx_count + tx) * BN_VEC;
  if (c0 >= C) return;
  float sc[BN_VEC], sh[BN_VEC];
  load8(scale + c0, sc);
  load8(shift + c0, sh);
  for (long mo = (long)blockIdx.x * rows_per_blk + ty; mo < Mo;
       mo += (long)gridDim.x * rows_per_blk) {
    const unsigned mm = (unsigned)mo;  // < 2^31, checked by the host
    const unsigned q = mm / (unsigned)p.Wo;
    const int wo = (int)(mm - q * (unsigned)p.Wo);
    const unsigned n = q / (unsigned)p.Ho;
    const int ho = (int)(q - n * (unsigned)p.Ho);
    Raw8<T> rx[9];
    bool ok[9];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int h = 2 * ho - 1 + kh;
      const int hc = min(max(h, 0), p.H - 1);
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int w = 2 * wo - 1 + kw;
        const int wc = min(max(w, 0), p.W - 1);
        ok[kh * 3 + kw] = h == hc && w == wc;
        rx[kh * 3 + kw] =
            load8raw(x + (((long)n * p.H + hc) * p.W + wc) * C + c0);
      }
    }
    float best[BN_VEC];
    unsigned idx[BN_VEC];
#pragma unroll
    for (int k = 0; k < BN_VEC; ++k) { best[k] = -1.f; idx[k] = 0; }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      float v[BN_VEC];
      unpack8(rx[j], v);
#pragma unroll
      for (int k = 0; k < BN_VEC; ++k) {
        float r = round_to(fmaxf(fmaf(v[k], sc[k], sh[k]), 0.f),
                           (const T*)nullptr);
        const bool take = ok[j] && r > best[k];
        best[k] = take ? r : best[k];
        idx[k] = take ? (unsigned)j : idx[k];
      }
    }
    unsigned word = 0;
#pragma unroll
    for (int k = 0; k < BN_VEC; ++k)
      word |= (best[k] > 0.f ? idx[k] : BN_POOL_NONE) << (4 * k);
    store8(y + mo * C + c0, best);
    amax[mo * (C / BN_VEC) + c0 / BN_VEC] = word;
  }
}

// ------------------------------------- fwd apply, block tail with two BNs
// y = relu(bn3(z) + bn_ds(zd)) and its packed mask. The inner value is
// rounded to T first: it is the identity tensor that the plain apply kernel
// would have stored and the ADD variant read back.
template <typename T>
__device__ __forceinline__ void bn_fwd_apply_add_bn_row(
    const Raw8<T>& rz, const Raw8<T>& rzd, const float* sc, const float* sh,
    const float* scd, const float* shd, T* __restrict__ y,
    unsigned char* __restrict__ mask, long m, int C, int c0) {
#pragma clang fp contract(off)
  float v[BN_VEC], r[BN_VEC];
  unpack8(rz, v);
  unpack8(rzd, r);
#pragma unroll
  for (int k = 0; k < BN_VEC; ++k) {
    v[k] = fmaf(v[k], sc[k], sh[k]);
    v[k] += round_to(fmaf(r[k], scd[k], shd[k]), (const T*)nullptr);
    v[k] = fmaxf(v[k], 0.f);
  }
  mask[m * (C / BN_VEC) + c0 / BN_VEC] =
      (unsigned char)store8_mask(y + m * C + c0, v);
}

template <typename T>
__global__ void __launch_bounds__(BLOCK_THREADS)
bn_fwd_apply_add_bn_kernel(
    const T* __restrict__ z, const T* __restrict__ zd, T* __restrict__ y,
    unsigned char* __restrict__ mask, const float* __restrict__ scale,
    const float* __restrict__ shift, const float* __restrict__ scale_d,
    const float* __restrict__ shift_d, long M, int C) {
  constexpr int U = BN_APPLY_FWD_U;
  int tx_count = min(C / BN_VEC, (int)blockDim.x);
  int tx = threadIdx.x % tx_count;
  int ty = threadIdx.x / tx_count;
  int rows_per_blk = blockDim.x / tx_count;
  int c0 = (blockIdx.y * tx_count + tx) * BN_VEC;
  if (c0 >= C) return;
  float sc[BN_VEC], sh[BN_VEC], scd[BN_VEC], shd[BN_VEC];
  load8(scale + c0, sc);
  load8(shift + c0, sh);
  load8(scale_d + c0, scd);
  load8(shift_d + c0, shd);
  const long stride = (long)gridDim.x * rows_per_blk;
  long m = (long)blockIdx.x * rows_per_blk + ty;
  if (U > 1) {
    for (; m + (U - 1) * stride < M; m += U * stride) {
      Raw8<T> rz[U], rzd[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        rz[u] = load8raw(z + (m + u * stride) * C + c0);
        rzd[u] = load8raw(zd + (m + u * stride) * C + c0);
      }
      // every load of the trip is issued before the first row is consumed
#pragma unroll
      for (int u = 0; u < U; ++u) {
        pin8(rz[u]);
        pin8(rzd[u]);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        bn_fwd_apply_add_bn_row<T>(rz[u], rzd[u], sc, sh, scd, shd, y, mask,
                                   m + u * stride, C, c0);
        __builtin_amdgcn_sched_barrier(0);  // see bn_fwd_apply_kernel
      }
    }
  }
  for (; m < M; m += stride)
    bn_fwd_apply_add_bn_row<T>(load8raw(z + m * C + c0),
                               load8raw(zd + m * C + c0), sc, sh, scd, shd, y,
                               mask, m, C, c0);
}

// ------------------------------------------------------------- bwd reduce
// dz = RELU ? (y>0 ? dy : 0) : dy ; accumulate sum_dz, sum_dz*xhat.
// RELU is BN_RELU_NONE, BN_RELU_Y (y > 0 from the stored y) or BN_RELU_MASK
// (the same bit, read from the forward's packed mask: 1 byte, not 8 values)
// or BN_RELU_POOL (dy is the pooled dy: dz is gathered through the argmax
// words of pool, see pool_issue / pool_dz).
template <typename T, int RELU>
__device__ __forceinline__ void bn_load_dz(const T* __restrict__ dy,
                                           const T* __restrict__ y,
                                           const unsigned char* __restrict__ mask,
                                           const BNPool& pool, long m, int C,
                                           int c0, float* dv) {
  if (RELU == BN_RELU_POOL) {
    PoolTaps<T> t;
    pool_issue(dy, pool, m, C, c0, t);
    pool_dz(t, dv);
    return;
  }
  load8(dy + m * C + c0, dv);
  if (RELU == BN_RELU_Y) {
    float yv[BN_VEC];
    load8(y + m * C + c0, yv);
#pragma unroll
    for (int k = 0; k < BN_VEC; ++k) dv[k] = yv[k] > 0.f ? dv[k] : 0.f;
  }
  if (RELU == BN_RELU_MASK)
    apply_mask8(mask[m * (C / BN_VEC) + c0 / BN_VEC], dv);
}

template <typename T, int RELU>
__global__ void __launch_bounds__(BLOCK_THREADS)
__attribute__((amdgpu_waves_per_eu(RELU == BN_RELU_POOL ? 2 : 1)))
bn_bwd_reduce_kernel(const T* __restrict__ x, const T* __restrict__ dy,
                     const T* __restrict__ y,
                     const unsigned char* __restrict__ mask,
                     const float* __restrict__ save_mean,
                     const float* __restrict__ save_rstd,
                     float* __restrict__ partial_dz,
                     float* __restrict__ partial_dzxh, long M, int C,
                     BNPool pool) {
#pragma clang fp contract(off)  // see bn_fwd_reduce_kernel
  int tx_count = min(C / BN_VEC, (int)blockDim.x);
  int tx = threadIdx.x % tx_count;
  int ty = threadIdx.x / tx_count;
  int rows_per_blk = blockDim.x / tx_count;
  int c0 = (blockIdx.y * tx_count + tx) * BN_VEC;
  if (c0 >= C) return;
  float mean[BN_VEC], rstd[BN_VEC];
  load8(save_mean + c0, mean);
  load8(save_rstd + c0, rstd);
  float s[BN_VEC] = {0}, t[BN_VEC] = {0};
  const long stride = (long)gridDim.x * rows_per_blk;
  long m = (long)blockIdx.x * rows_per_blk + ty;
  for (; m + (BN_RED_U - 1) * stride < M; m += BN_RED_U * stride) {
    Raw8<T> rx[BN_RED_U], rd[BN_RED_U], ry[BN_RED_U];
    unsigned rm[BN_RED_U];
    PoolTaps<T> rp[BN_RED_U];
#pragma unroll
    for (int u = 0; u < BN_RED_U; ++u) {
      const long mu = m + u * stride;
      rx[u] = load8raw(x + mu * C + c0);
      if (RELU == BN_RELU_POOL) {
        pool_issue(dy, pool, mu, C, c0, rp[u]);
        // issue this row's nine loads before the next row's addresses are
        // formed: 36 addresses held at once cost more registers than the data
        __builtin_amdgcn_sched_barrier(0);
      } else {
        rd[u] = load8raw(dy + mu * C + c0);
      }
      if (RELU == BN_RELU_Y) ry[u] = load8raw(y + mu * C + c0);
      if (RELU == BN_RELU_MASK) rm[u] = mask[mu * (C / BN_VEC) + c0 / BN_VEC];
    }
    // every load of the trip is issued before the first row is consumed
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < BN_RED_U; ++u) {
      float xv[BN_VEC], dv[BN_VEC];
      unpack8(rx[u], xv);
      if (RELU == BN_RELU_POOL) pool_dz(rp[u], dv);
      else unpack8(rd[u], dv);
      if (RELU == BN_RELU_Y) {
        float yv[BN_VEC];
        unpack8(ry[u], yv);
#pragma unroll
        for (int k = 0; k < BN_VEC; ++k) dv[k] = yv[k] > 0.f ? dv[k] : 0.f;
      }
      if (RELU == BN_RELU_MASK) apply_mask8(rm[u], dv);
#pragma unroll
      for (int k = 0; k < BN_VEC; ++k) {
        s[k] += dv[k];
        t[k] = fmaf(dv[k] * (xv[k] - mean[k]), rstd[k], t[k]);
      }
      // one row's taps unpacked at a time: interleaved, the four rows' 128
      // unpacked values do not fit beside the loads still in flight
      if (RELU == BN_RELU_POOL) __builtin_amdgcn_sched_barrier(0);
    }
  }
  for (; m < M; m += stride) {
    float xv[BN_VEC], dv[BN_VEC];
    load8(x + m * C + c0, xv);
    bn_load_dz<T, RELU>(dy, y, mask, pool, m, C, c0, dv);
#pragma unroll
    for (int k = 0; k < BN_VEC; ++k) {
      s[k] += dv[k];
      t[k] = fmaf(dv[k] * (xv[k] - mean[k]), rstd[k], t[k]);
    }
  }
  __shared__ float ls[BLOCK_THREADS * BN_VEC];
  __shared__ float lt[BLOCK_THREADS * BN_VEC];
#pragma unroll
  for (int k = 0; k < BN_VEC; ++k) {
    ls[threadIdx.x * BN_VEC + k] = s[k];
    lt[threadIdx.x * BN_VEC + k] = t[k];
  }
  __syncthreads();
  if (ty == 0) {
    for (int r = 1; r < rows_per_blk; ++r) {
      int o = (r * tx_count + tx) * BN_VEC;
#pragma unroll
      for (int k = 0; k < BN_VEC; ++k) { s[k] += ls[o + k]; t[k] += lt[o + k]; }
    }
    store8(partial_dz + (long)blockIdx.x * C + c0, s);
    store8(partial_dzxh + (long)blockIdx.x * C + c0, t);
  }
}

// ----------------------------------------------- bwd reduce, two gradients
// The tail of a residual block gets its dy as two addends (the block output
// feeds the next block's conv1 and its residual / downsample conv). This is
// the BN_RELU_MASK reduce with the add folded in:
//   dz = bit ? T(float(a) + float(b)) : 0
// one fp32 add rounded to T, which is torch's a + b, then the mask. The sums
// are taken from the rounded, masked value with the expressions and in the
// order of bn_bwd_reduce_kernel, so the partial rows are those of that kernel
// on dy = a + b. dz is stored: it is the dres of the split path, and
// bn_bwd_apply_kernel<T, BN_RELU_NONE, false> on dy = dz gives its dx.
// BN_JOIN_U rows in flight: 3 streams of 16 B and the mask byte per row.
#ifndef BN_JOIN_U
#define BN_JOIN_U 4
#endif
template <typename T>
__device__ __forceinline__ void bn_join_dz8(const float* av, const float* bv,
                                            unsigned bits, float* dv) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < BN_VEC; ++k)
    dv[k] = (bits >> k) & 1u ? round_to(av[k] + bv[k], (const T*)nullptr)
                             : 0.f;
}

template <typename T>
__global__ void __launch_bounds__(BLOCK_THREADS)
__attribute__((amdgpu_waves_per_eu(1)))
bn_bwd_reduce_join_kernel(const T* __restrict__ x, const T* __restrict__ dy_a,
                          const T* __restrict__ dy_b,
                          const unsigned char* __restrict__ mask,
                          const float* __restrict__ save_mean,
                          const float* __restrict__ save_rstd,
                          float* __restrict__ partial_dz,
                          float* __restrict__ partial_dzxh,
                          T* __restrict__ dz, long M, int C) {
#pragma clang fp contract(off)  // see bn_fwd_reduce_kernel
  int tx_count = min(C / BN_VEC, (int)blockDim.x);
  int tx = threadIdx.x % tx_count;
  int ty = threadIdx.x / tx_count;
  int rows_per_blk = blockDim.x / tx_count;
  int c0 = (blockIdx.y * tx_count + tx) * BN_VEC;
  if (c0 >= C) return;
  float mean[BN_VEC], rstd[BN_VEC];
  load8(save_mean + c0, mean);
  load8(save_rstd + c0, rstd);
  float s[BN_VEC] = {0}, t[BN_VEC] = {0};
  const long stride = (long)gridDim.x * rows_per_blk;
  long m = (long)blockIdx.x * rows_per_blk + ty;
  for (; m + (BN_JOIN_U - 1) * stride < M; m += BN_JOIN_U * stride) {
    Raw8<T> rx[BN_JOIN_U], ra[BN_JOIN_U], rb[BN_JOIN_U];
    unsigned rm[BN_JOIN_U];
#pragma unroll
    for (int u = 0; u < BN_JOIN_U; ++u) {
      const long mu = m + u * stride;
      rx[u] = load8raw(x + mu * C + c0);
      ra[u] = load8raw(dy_a + mu * C + c0);
      rb[u] = load8raw(dy_b + mu * C + c0);
      rm[u] = mask[mu * (C / BN_VEC) + c0 / BN_VEC];
    }
    // every load of the trip is issued before the first row is consumed
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < BN_JOIN_U; ++u) {
      float xv[BN_VEC], av[BN_VEC], bv[BN_VEC], dv[BN_VEC];
      unpack8(rx[u], xv);
      unpack8(ra[u], av);
      unpack8(rb[u], bv);
      bn_join_dz8<T>(av, bv, rm[u], dv);
#pragma unroll
      for (int k = 0; k < BN_VEC; ++k) {
        s[k] += dv[k];
        t[k] = fmaf(dv[k] * (xv[k] - mean[k]), rstd[k], t[k]);
      }
      store8(dz + (m + u * stride) * C + c0, dv);
    }
  }
  for (; m < M; m += stride) {
    float xv[BN_VEC], av[BN_VEC], bv[BN_VEC], dv[BN_VEC];
    load8(x + m * C + c0, xv);
    load8(dy_a + m * C + c0, av);
    load8(dy_b + m * C + c0, bv);
    bn_join_dz8<T>(av, bv, mask[m * (C / BN_VEC) + c0 / BN_VEC], dv);
#pragma unroll
    for (int k = 0; k < BN_VEC; ++k) {
      s[k] += dv[k];
      t[k] = fmaf(dv[k] * (xv[k] - mean[k]), rstd[k], t[k]);
    }
    store8(dz + m * C + c0, dv);
  }
  __shared__ float ls[BLOCK_THREADS * BN_VEC];
  __shared__ float lt[BLOCK_THREADS * BN_VEC];
#pragma unroll
  for (int k = 0; k < BN_VEC; ++k) {
    ls[threadIdx.x * BN_VEC + k] = s[k];
    lt[threadIdx.x * BN_VEC + k] = t[k];
  }
  __syncthreads();
  if (ty == 0) {
    for (int r = 1; r < rows_per_blk; ++r) {
      int o = (r * tx_count + tx) * BN_VEC;
#pragma unroll
      for (int k = 0; k < BN_VEC; ++k) { s[k] += ls[o + k]; t[k] += lt[o + k]; }
    }
    store8(partial_dz + (long)blockIdx.x * C + c0, s);
    store8(partial_dzxh + (long)blockIdx.x * C + c0, t);
  }
}

// ------------------------------- bwd reduce, two gradients and two branches
// The tail relu(bn3(z) + bn_ds(zd)) of a block with a downsample: both BNs
// get the same dz, so one pass forms it (as bn_bwd_reduce_join_kernel does),
// stores it, and takes sum dz once and sum dz*xhat of each branch. Grid, rows
// per thread, order and expressions are those of bn_bwd_reduce_join_kernel on
// z and of bn_bwd_reduce_kernel<T, BN_RELU_NONE> on (zd, dz), so each of the
// three partial matrices is what those kernels write, bit for bit.
// BN_JOIN2_U rows in flight: 4 streams of 16 B and the mask byte per row.
#ifndef BN_JOIN2_U
#define BN_JOIN2_U 2
#endif
template <typename T>
__global__ void __launch_bounds__(BLOCK_THREADS)
__attribute__((amdgpu_waves_per_eu(1)))
bn_bwd_reduce_join2_kernel(const T* __restrict__ z, const T* __restrict__ zd,
                           const T* __restrict__ dy_a,
                           const T* __restrict__ dy_b,
                           const unsigned char* __restrict__ mask,
                           const float* __restrict__ save_mean,
                           const float* __restrict__ save_rstd,
                           const float* __restrict__ save_mean_d,
                           const float* __restrict__ save_rstd_d,
                           float* __restrict__ partial_dz,
                           float* __restrict__ partial_dzxh,
                           float* __restrict__ partial_dzxh_d,
                           T* __restrict__ dz, long M, int C) {
#pragma clang fp contract(off)  // see bn_fwd_reduce_kernel
  int tx_count = min(C / BN_VEC, (int)blockDim.x);
  int tx = threadIdx.x % tx_count;
  int ty = threadIdx.x / tx_count;
  int rows_per_blk = blockDim.x / tx_count;
  int c0 = (blockIdx.y * tx_count + tx) * BN_VEC;
  if (c0 >= C) return;
  float mean[BN_VEC], rstd[BN_VEC], mean_d[BN_VEC], rstd_d[BN_VEC];
  load8(save_mean + c0, mean);
  load8(save_rstd + c0, rstd);
  load8(save_mean_d + c0, mean_d);
  load8(save_rstd_d + c0, rstd_d);
  float s[BN_VEC] = {0}, t[BN_VEC] = {0}, td[BN_VEC] = {0};
  const long stride = (long)gridDim.x * rows_per_blk;
  long m = (long)blockIdx.x * rows_per_blk + ty;
  for (; m + (BN_JOIN2_U - 1) * stride < M; m += BN_JOIN2_U * stride) {
    Raw8<T> rz[BN_JOIN2_U], rzd[BN_JOIN2_U], ra[BN_JOIN2_U], rb[BN_JOIN2_U];
    unsigned rm[BN_JOIN2_U];
#pragma unroll
    for (int u = 0; u < BN_JOIN2_U; ++u) {
      const long mu = m + u * stride;
      rz[u] = load8raw(z + mu * C + c0);
      rzd[u] = load8raw(zd + mu * C + c0);
      ra[u] = load8raw(dy_a + mu * C + c0);
      rb[u] = load8raw(dy_b + mu * C + c0);
      rm[u] = mask[mu * (C / BN_VEC) + c0 / BN_VEC];
    }
    // every load of the trip is issued before the first row is consumed
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < BN_JOIN2_U; ++u) {
      float zv[BN_VEC], zdv[BN_VEC], av[BN_VEC], bv[BN_VEC], dv[BN_VEC];
      unpack8(rz[u], zv);
      unpack8(rzd[u], zdv);
      unpack8(ra[u], av);
      unpack8(rb[u], bv);
      bn_join_dz8<T>(av, bv, rm[u], dv);
#pragma unroll
      for (int k = 0; k < BN_VEC; ++k) {
        s[k] += dv[k];
        t[k] = fmaf(dv[k] * (zv[k] - mean[k]), rstd[k], t[k]);
        td[k] = fmaf(dv[k] * (zdv[k] - mean_d[k]), rstd_d[k], td[k]);
      }
      store8(dz + (m + u * stride) * C + c0, dv);
    }
  }
  for (; m < M; m += stride) {
    float zv[BN_VEC], zdv[BN_VEC], av[BN_VEC], bv[BN_VEC], dv[BN_VEC];
    load8(z + m * C + c0, zv);
    load8(zd + m * C + c0, zdv);
    load8(dy_a + m * C + c0, av);
    load8(dy_b + m * C + c0, bv);
    bn_join_dz8<T>(av, bv, mask[m * (C / BN_VEC) + c0 / BN_VEC], dv);
#pragma unroll
    for (int k = 0; k < BN_VEC; ++k) {
      s[k] += dv[k];
      t[k] = fmaf(dv[k] * (zv[k] - mean[k]), rstd[k], t[k]);
      td[k] = fmaf(dv[k] * (zdv[k] - mean_d[k]), rstd_d[k], td[k]);
    }
    store8(dz + m * C + c0, dv);
  }
  __shared__ float ls[BLOCK_THREADS * BN_VEC];
  __shared__ float lt[BLOCK_THREADS * BN_VEC];
  __shared__ float ltd[BLOCK_THREADS * BN_VEC];
#pragma unroll
  for (int k = 0; k < BN_VEC; ++k) {
    ls[threadIdx.x * BN_VEC + k] = s[k];
    lt[threadIdx.x * BN_VEC + k] = t[k];
    ltd[threadIdx.x * BN_VEC + k] = td[k];
  }
  __syncthreads();
  if (ty == 0) {
    for (int r = 1; r < rows_per_blk; ++r) {
      int o = (r * tx_count + tx) * BN_VEC;
#pragma unroll
      for (int k = 0; k < BN_VEC; ++k) {
        s[k] += ls[o + k];
        t[k] += lt[o + k];
        td[k] += ltd[o + k];
      }
    }
    store8(partial_dz + (long)blockIdx.x * C + c0, s);
    store8(partial_dzxh + (long)blockIdx.x * C + c0, t);
    store8(partial_dzxh_d + (long)blockIdx.x * C + c0, td);
  }
}

// ------------------------------------------------------------ bwd finalize
// k1 = w*rstd ; k2 = sum_dz/M ; k3 = sum_dzxh/M ; dweight = sum_dzxh ;
// dbias = sum_dz
__global__ void bn_bwd_finalize_kernel(const float* __restrict__ partial_dz,
                                       const float* __restrict__ partial_dzxh,
                                       int grid_m,
                                       const float* __restrict__ weight,
                                       const float* __restrict__ save_rstd,
                                       float* __restrict__ k1,
                                       float* __restrict__ k2,
                                       float* __restrict__ k3,
                                       float* __restrict__ dweight,
                                       float* __restrict__ dbias, long M,
                                       int C) {
  int tx = threadIdx.x % FIN_CH;
  int ty = threadIdx.x / FIN_CH;
  int c = blockIdx.x * FIN_CH + tx;
  if (c >= C) return;
  float sdz = 0.f, sdzxh = 0.f;
  bn_fin_lane_sum(partial_dz, partial_dzxh, grid_m, ty, C, c, sdz, sdzxh);
  __shared__ float ls[FIN_LANES * FIN_CH], lq[FIN_LANES * FIN_CH];
  ls[ty * FIN_CH + tx] = sdz;
  lq[ty * FIN_CH + tx] = sdzxh;
  __syncthreads();
  if (ty != 0) return;
#pragma unroll
  for (int r = 1; r < FIN_LANES; ++r) {
    sdz += ls[r * FIN_CH + tx];
    sdzxh += lq[r * FIN_CH + tx];
  }
  k1[c] = weight[c] * save_rstd[c];
  k2[c] = sdz / (float)M;
  k3[c] = sdzxh / (float)M;
  dweight[c] = sdzxh;
  dbias[c] = sdz;
}

// -------------------------------------------------------------- bwd apply
// dx = k1*(dz - k2 - xhat*k3); dres = dz (if ADD)
// Spelled as the one-row loop compiled it, contraction off (see
// bn_fwd_apply_kernel): dz - k2 - xhat*k3 had become one fma on -xhat.
__device__ __forceinline__ void bn_bwd_dx8(const float* xv, const float* dv,
                                           const float* mean,
                                           const float* rstd, const float* a1,
                                           const float* a2, const float* a3,
                                           float* o) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < BN_VEC; ++k) {
    float xhat = (xv[k] - mean[k]) * rstd[k];
    o[k] = a1[k] * fmaf(-xhat, a3[k], dv[k] - a2[k]);
  }
}

// The pool variant keeps its one-row loop: its nine gathered loads per row
// are in flight already.
template <typename T, int RELU, bool ADD>
__global__ void
__launch_bounds__(RELU == BN_RELU_POOL ? 1024 : BLOCK_THREADS)
bn_bwd_apply_kernel(const T* __restrict__ x,
                                    const T* __restrict__ dy,
                                    const T* __restrict__ y,
                                    const unsigned char* __restrict__ mask,
                                    const float* __restrict__ save_mean,
                                    const float* __restrict__ save_rstd,
                                    const float* __restrict__ k1,
                                    const float* __restrict__ k2,
                                    const float* __restrict__ k3,
                                    T* __restrict__ dx, T* __restrict__ dres,
                                    long M, int C, BNPool pool) {
  int tx_count = min(C / BN_VEC, (int)blockDim.x);
  int tx = threadIdx.x % tx_count;
  int ty = threadIdx.x / tx_count;
  int rows_per_blk = blockDim.x / tx_count;
  int c0 = (blockIdx.y * tx_count + tx) * BN_VEC;
  if (c0 >= C) return;
  float mean[BN_VEC], rstd[BN_VEC], a1[BN_VEC], a2[BN_VEC], a3[BN_VEC];
  load8(save_mean + c0, mean);
  load8(save_rstd + c0, rstd);
  load8(k1 + c0, a1);
  load8(k2 + c0, a2);
  load8(k3 + c0, a3);
  if (RELU == BN_RELU_POOL) {
    for (long m = (long)blockIdx.x * rows_per_blk + ty; m < M;
         m += (long)gridDim.x * rows_per_blk) {
      float xv[BN_VEC], dv[BN_VEC];
      load8(x + m * C + c0, xv);
      bn_load_dz<T, RELU>(dy, y, mask, pool, m, C, c0, dv);
      if (ADD) store8(dres + m * C + c0, dv);
      float o[BN_VEC];
#pragma unroll
      for (int k = 0; k < BN_VEC; ++k) {
        float xhat = (xv[k] - mean[k]) * rstd[k];
        o[k] = a1[k] * (dv[k] - a2[k] - xhat * a3[k]);
      }
      store8(dx + m * C + c0, o);
    }
    return;
  }
  constexpr int U = BN_APPLY_BWD_U;
  const long stride = (long)gridDim.x * rows_per_blk;
  long m = (long)blockIdx.x * rows_per_blk + ty;
  if (U > 1) {
    for (; m + (U - 1) * stride < M; m += U * stride) {
      Raw8<T> rx[U], rd[U], ry[U];
      unsigned rm[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long mu = m + u * stride;
        rx[u] = load8raw(x + mu * C + c0);
        rd[u] = load8raw(dy + mu * C + c0);
        if (RELU == BN_RELU_Y) ry[u] = load8raw(y + mu * C + c0);
        if (RELU == BN_RELU_MASK)
          rm[u] = mask[mu * (C / BN_VEC) + c0 / BN_VEC];
      }
      // every load of the trip is issued before the first row is consumed
#pragma unroll
      for (int u = 0; u < U; ++u) {
        pin8(rx[u]);
        pin8(rd[u]);
        if (RELU == BN_RELU_Y) pin8(ry[u]);
        if (RELU == BN_RELU_MASK) pin8(rm[u]);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long mu = m + u * stride;
        float xv[BN_VEC], dv[BN_VEC], o[BN_VEC];
        unpack8(rx[u], xv);
        unpack8(rd[u], dv);
        if (RELU == BN_RELU_Y) {
          float yv[BN_VEC];
          unpack8(ry[u], yv);
#pragma unroll
          for (int k = 0; k < BN_VEC; ++k) dv[k] = yv[k] > 0.f ? dv[k] : 0.f;
        }
        if (RELU == BN_RELU_MASK) apply_mask8(rm[u], dv);
        if (ADD) store8(dres + mu * C + c0, dv);
        bn_bwd_dx8(xv, dv, mean, rstd, a1, a2, a3, o);
        store8(dx + mu * C + c0, o);
        __builtin_amdgcn_sched_barrier(0);  // see bn_fwd_apply_kernel
      }
    }
  }
  for (; m < M; m += stride) {
    float xv[BN_VEC], dv[BN_VEC], o[BN_VEC];
    load8(x + m * C + c0, xv);
    bn_load_dz<T, RELU>(dy, y, mask, pool, m, C, c0, dv);
    if (ADD) store8(dres + m * C + c0, dv);
    bn_bwd_dx8(xv, dv, mean, rstd, a1, a2, a3, o);
    store8(dx + m * C + c0, o);
  }
}

// ------------------------------------------------- bwd apply, two branches
// The apply of the relu(bn3(z) + bn_ds(zd)) tail: one read of dz (already
// masked, written by bn_bwd_reduce_join2_kernel) gives dx of both branches,
// each with the arithmetic of bn_bwd_apply_kernel<T, BN_RELU_NONE, false>.
// k2 = sum dz / M is one value for both branches.
template <typename T>
__global__ void __launch_bounds__(BLOCK_THREADS)
bn_bwd_apply2_kernel(const T* __restrict__ z, const T* __restrict__ zd,
                     const T* __restrict__ dz,
                     const float* __restrict__ save_mean,
                     const float* __restrict__ save_rstd,
                     const float* __restrict__ save_mean_d,
                     const float* __restrict__ save_rstd_d,
                     const float* __restrict__ k1, const float* __restrict__ k2,
                     const float* __restrict__ k3,
                     const float* __restrict__ k1_d,
                     const float* __restrict__ k3_d, T* __restrict__ dx,
                     T* __restrict__ dx_d, long M, int C) {
  constexpr int U = BN_APPLY2_U;
  int tx_count = min(C / BN_VEC, (int)blockDim.x);
  int tx = threadIdx.x % tx_count;
  int ty = threadIdx.x / tx_count;
  int rows_per_blk = blockDim.x / tx_count;
  int c0 = (blockIdx.y * tx_count + tx) * BN_VEC;
  if (c0 >= C) return;
  float mean[BN_VEC], rstd[BN_VEC], a1[BN_VEC], a2[BN_VEC], a3[BN_VEC];
  float mean_d[BN_VEC], rstd_d[BN_VEC], a1_d[BN_VEC], a3_d[BN_VEC];
  load8(save_mean + c0, mean);
  load8(save_rstd + c0, rstd);
  load8(k1 + c0, a1);
  load8(k2 + c0, a2);
  load8(k3 + c0, a3);
  load8(save_mean_d + c0, mean_d);
  load8(save_rstd_d + c0, rstd_d);
  load8(k1_d + c0, a1_d);
  load8(k3_d + c0, a3_d);
  const long stride = (long)gridDim.x * rows_per_blk;
  long m = (long)blockIdx.x * rows_per_blk + ty;
  if (U > 1) {
    for (; m + (U - 1) * stride < M; m += U * stride) {
      Raw8<T> rz[U], rzd[U], rd[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long mu = m + u * stride;
        rz[u] = load8raw(z + mu * C + c0);
        rzd[u] = load8raw(zd + mu * C + c0);
        rd[u] = load8raw(dz + mu * C + c0);
      }
      // every load of the trip is issued before the first row is consumed
#pragma unroll
      for (int u = 0; u < U; ++u) {
        pin8(rz[u]);
        pin8(rzd[u]);
        pin8(rd[u]);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long mu = m + u * stride;
        float zv[BN_VEC], zdv[BN_VEC], dv[BN_VEC], o[BN_VEC];
        unpack8(rz[u], zv);
        unpack8(rzd[u], zdv);
        unpack8(rd[u], dv);
        bn_bwd_dx8(zv, dv, mean, rstd, a1, a2, a3, o);
        store8(dx + mu * C + c0, o);
        bn_bwd_dx8(zdv, dv, mean_d, rstd_d, a1_d, a2, a3_d, o);
        store8(dx_d + mu * C + c0, o);
        __builtin_amdgcn_sched_barrier(0);  // see bn_fwd_apply_kernel
      }
    }
  }
  for (; m < M; m += stride) {
    float zv[BN_VEC], zdv[BN_VEC], dv[BN_VEC], o[BN_VEC];
    load8(z + m * C + c0, zv);
    load8(zd + m * C + c0, zdv);
    load8(dz + m * C + c0, dv);
    bn_bwd_dx8(zv, dv, mean, rstd, a1, a2, a3, o);
    store8(dx + m * C + c0, o);
    bn_bwd_dx8(zdv, dv, mean_d, rstd_d, a1_d, a2, a3_d, o);
    store8(dx_d + m * C + c0, o);
  }
}
