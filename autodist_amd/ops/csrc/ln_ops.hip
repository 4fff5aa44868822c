// Fused LayerNorm (+ residual add) for bf16 transformer streams, gfx950.
//
// torch's LN on a bf16 autocast stream runs fp32 kernels bracketed by
// bfloat16<->float32 copy kernels (measured: the cast/elementwise cluster
// around LN was ~13% of the BERT-base step). These kernels read/write
// bf16 directly with fp32 accumulation, and fold the residual add
// y = LN(a + b) into the same pass (saving the separate add kernel AND
// its extra HBM round trip). Saved for backward: the summed input u
// (bf16, doubles as the residual stream), mean and rstd (fp32 per row).
//
// Shapes: x [N, H] rows normalized over H; H <= 256 * LN_MAX_PER_THREAD
// and H % 2 == 0 (bf16 pairs). One 256-thread block per row; row sums
// via DPP 16-lane reduction + 2 cross-group shuffles + LDS across the 4
// waves.
#include "common.h"

#define LN_MAX_PER_THREAD 16  // H up to 4096

typedef short ln_bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float ln_wave_sum(float v) {
  v = dpp16_sum(v);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// block-wide sum of two values at once (saves one barrier round)
__device__ __forceinline__ void ln_block_sum2(float& a, float& b,
                                              float* lds /* >= 8 */) {
  int w = threadIdx.x >> 6;
  a = ln_wave_sum(a);
  b = ln_wave_sum(b);
  if ((threadIdx.x & 63) == 0) {
    lds[w] = a;
    lds[4 + w] = b;
  }
  __syncthreads();
  a = lds[0] + lds[1] + lds[2] + lds[3];
  b = lds[4] + lds[5] + lds[6] + lds[7];
  __syncthreads();
}

// paired (bf16x2) loads/stores: H must be even (the module guards)
__global__ void
__launch_bounds__(256)
ln_fwd_kernel(const __hip_bfloat16* __restrict__ x,
              const __hip_bfloat16* __restrict__ res,  // nullable
              const float* __restrict__ gamma, const float* __restrict__ beta,
              __hip_bfloat16* __restrict__ y,
              __hip_bfloat16* __restrict__ u_out,      // nullable
              float* __restrict__ mean_out, float* __restrict__ rstd_out,
              long N, int H, float eps) {
  __shared__ float lds[8];
  long row = blockIdx.x;
  if (row >= N) return;
  const __hip_bfloat162* xr =
      reinterpret_cast<const __hip_bfloat162*>(x + row * H);
  const __hip_bfloat162* rr = res
      ? reinterpret_cast<const __hip_bfloat162*>(res + row * H) : nullptr;
  int H2 = H >> 1;
  float2 v[LN_MAX_PER_THREAD / 2];
  int nper = (H2 + 255) >> 8;
  float acc = 0.f, acc2 = 0.f;
  for (int k = 0; k < nper; ++k) {
    int i = threadIdx.x + (k << 8);
    float2 u = {0.f, 0.f};
    if (i < H2) {
      u = __bfloat1622float2(xr[i]);
      if (rr) {
        float2 r2 = __bfloat1622float2(rr[i]);
        u.x += r2.x;
        u.y += r2.y;
      }
    }
    v[k] = u;
    acc += u.x + u.y;
    acc2 += u.x * u.x + u.y * u.y;
  }
  ln_block_sum2(acc, acc2, lds);
  float mean = acc / H;
  float var = fmaxf(acc2 / H - mean * mean, 0.f);
  float rstd = rsqrtf(var + eps);
  if (threadIdx.x == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
  __hip_bfloat162* yr = reinterpret_cast<__hip_bfloat162*>(y + row * H);
  __hip_bfloat162* ur = u_out
      ? reinterpret_cast<__hip_bfloat162*>(u_out + row * H) : nullptr;
  const float2* g2 = reinterpret_cast<const float2*>(gamma);
  const float2* b2 = reinterpret_cast<const float2*>(beta);
  for (int k = 0; k < nper; ++k) {
    int i = threadIdx.x + (k << 8);
    if (i < H2) {
      float2 gg = g2[i], bb = b2[i];
      float2 o = {(v[k].x - mean) * rstd * gg.x + bb.x,
                  (v[k].y - mean) * rstd * gg.y + bb.y};
      yr[i] = __float22bfloat162_rn(o);
      if (ur) ur[i] = __float22bfloat162_rn(v[k]);
    }
  }
}

// dx = rstd * (g - mean(g) - xhat * mean(g*xhat)), g = dy*gamma (fp32)
__global__ void
__launch_bounds__(256)
ln_bwd_dx_kernel(const __hip_bfloat16* __restrict__ dy,
                 const __hip_bfloat16* __restrict__ u,
                 const float* __restrict__ gamma,
                 const float* __restrict__ mean_in,
                 const float* __restrict__ rstd_in,
                 __hip_bfloat16* __restrict__ dx, long N, int H) {
  __shared__ float lds[8];
  long row = blockIdx.x;
  if (row >= N) return;
  const __hip_bfloat162* dyr =
      reinterpret_cast<const __hip_bfloat162*>(dy + row * H);
  const __hip_bfloat162* ur =
      reinterpret_cast<const __hip_bfloat162*>(u + row * H);
  const float2* g2 = reinterpret_cast<const float2*>(gamma);
  float mean = mean_in[row], rstd = rstd_in[row];
  int H2 = H >> 1;
  float2 g[LN_MAX_PER_THREAD / 2], xh[LN_MAX_PER_THREAD / 2];
  int nper = (H2 + 255) >> 8;
  float c1 = 0.f, c2 = 0.f;
  for (int k = 0; k < nper; ++k) {
    int i = threadIdx.x + (k << 8);
    float2 gv = {0.f, 0.f}, xv = {0.f, 0.f};
    if (i < H2) {
      float2 d2 = __bfloat1622float2(dyr[i]);
      float2 u2 = __bfloat1622float2(ur[i]);
      float2 gg = g2[i];
      gv = {d2.x * gg.x, d2.y * gg.y};
      xv = {(u2.x - mean) * rstd, (u2.y - mean) * rstd};
    }
    g[k] = gv;
    xh[k] = xv;
    c1 += gv.x + gv.y;
    c2 += gv.x * xv.x + gv.y * xv.y;
  }
  ln_block_sum2(c1, c2, lds);
  c1 /= H;
  c2 /= H;
  __hip_bfloat162* dxr = reinterpret_cast<__hip_bfloat162*>(dx + row * H);
  for (int k = 0; k < nper; ++k) {
    int i = threadIdx.x + (k << 8);
    if (i < H2) {
      float2 o = {rstd * (g[k].x - c1 - xh[k].x * c2),
                  rstd * (g[k].y - c1 - xh[k].y * c2)};
      dxr[i] = __float22bfloat162_rn(o);
    }
  }
}

// per-chunk partial dgamma/dbeta: grid (H/64, nchunks); 256 threads =
// 64 cols x 4 row-lanes; partials [nchunks, 2, H] fp32 summed by caller.
__global__ void
__launch_bounds__(256)
ln_bwd_gb_kernel(const __hip_bfloat16* __restrict__ dy,
                 const __hip_bfloat16* __restrict__ u,
                 const float* __restrict__ mean_in,
                 const float* __restrict__ rstd_in,
                 float* __restrict__ partials, long N, int H,
                 long rows_per_chunk) {
  __shared__ float pg[4][64];
  __shared__ float pb[4][64];
  int col = (blockIdx.x << 6) + (threadIdx.x & 63);
  int rl = threadIdx.x >> 6;  // row-lane 0..3
  long r0 = (long)blockIdx.y * rows_per_chunk;
  long r1 = min(r0 + rows_per_chunk, N);
  float sg = 0.f, sb = 0.f;
  if (col < H) {
    for (long r = r0 + rl; r < r1; r += 4) {
      float d = __bfloat162float(dy[r * H + col]);
      float xh = (__bfloat162float(u[r * H + col]) - mean_in[r]) * rstd_in[r];
      sg += d * xh;
      sb += d;
    }
  }
  pg[rl][threadIdx.x & 63] = sg;
  pb[rl][threadIdx.x & 63] = sb;
  __syncthreads();
  if (rl == 0 && col < H) {
    int c = threadIdx.x & 63;
    float tg = pg[0][c] + pg[1][c] + pg[2][c] + pg[3][c];
    float tb = pb[0][c] + pb[1][c] + pb[2][c] + pb[3][c];
    partials[((long)blockIdx.y * 2) * H + col] = tg;
    partials[((long)blockIdx.y * 2 + 1) * H + col] = tb;
  }
}

// column sum of a bf16 [N, H] matrix -> fp32 partials [nchunks, H]
// (bias gradients: torch's generic reduce_kernel<BFloat16> ran at
// ~0.35 TB/s on these shapes; this streams rows coalesced per column
// block and lets the caller sum the small partial matrix).
__global__ void
__launch_bounds__(256)
col_sum_kernel(const __hip_bfloat16* __restrict__ x,
               float* __restrict__ partials, long N, long H,
               long rows_per_chunk) {
  __shared__ float ps[4][64];
  long col = ((long)blockIdx.x << 6) + (threadIdx.x & 63);
  int rl = threadIdx.x >> 6;  // row-lane 0..3
  long r0 = (long)blockIdx.y * rows_per_chunk;
  long r1 = min(r0 + rows_per_chunk, N);
  float s = 0.f;
  if (col < H) {
    for (long r = r0 + rl; r < r1; r += 4) {
      s += __bfloat162float(x[r * H + col]);
    }
  }
  ps[rl][threadIdx.x & 63] = s;
  __syncthreads();
  if (rl == 0 && col < H) {
    int c = threadIdx.x & 63;
    partials[(long)blockIdx.y * H + col] =
        ps[0][c] + ps[1][c] + ps[2][c] + ps[3][c];
  }
}

// ---------------------------------------------------------------------------
// Fused dropout + residual + LayerNorm: y = LN(dropout_p(x) + res).
//
// Hidden dropout of a transformer sublayer folded into the norm that follows
// it. Element (row, col) is kept iff drop_hash(seed, 0, row, col) >=
// drop_thresh(p), the attention kernels' hash and threshold, so the backward
// regenerates the mask and nothing but u / mean / rstd is held for it.
//
// Geometry (H % 8 == 0, 8 <= H <= 4096, 16-byte aligned rows): every access
// is 16 bytes (8 bf16) per lane. A row belongs to a lane group of G lanes,
// G = 64 / 128 / 256 from H / 8 vectors, each lane holding V = 1 or 2 vectors
// (lane gl owns vectors gl and gl + G); a 256-thread block takes 256 / G rows.
// G = 64 reduces inside one wave (DPP + two shuffles, no LDS, no barrier);
// the wider groups fold their 2 or 4 wave sums through 8 LDS floats.
//
// Rounding points: u = x * keep * 1/(1-p) + res stays fp32 for the row
// statistics and y; it is rounded once to bf16 for the backward. The
// backward forms dU in fp32, stores dres = bf16(dU) and
// dx = keep ? bf16(dU * 1/(1-p)) : 0 from the unrounded dU.
//
// dgamma / dbeta: a lane owns fixed columns, so the backward keeps dy and
// dy * xhat column sums in registers across the rows its block walks (grid
// capped at LND_BWD_GRID_MAX, rows ascending), folds the block's row groups
// through LDS in group order and writes one partial row [2, H]; the finalize
// kernel adds the partial rows in a fixed order. No atomics: the result is
// bit-reproducible.
#define LND_NOPK __attribute__((target("no-packed-fp32-ops")))
#define LND_BWD_GRID_MAX 512
#define LND_FIN_COLS 32
#define LND_FIN_SLICES 8
#define LND_FIN_U 16  // partial rows in flight per finalize thread

// Header helpers that are plain `inline` (__uint_as_float, __float2bfloat16,
// make_uint4, __syncthreads) lack the target attribute and would stay calls
// inside these kernels, so the few that are needed are spelled out here.
__device__ __forceinline__ LND_NOPK float lnd_bits(unsigned int w) {
  return __builtin_bit_cast(float, w);
}

// the 8 bf16 of one 16-byte access, widened (exact)
__device__ __forceinline__ LND_NOPK void lnd_unpack8(const uint4& w,
                                                     float* x) {
  x[0] = lnd_bits(w.x << 16); x[1] = lnd_bits(w.x & 0xffff0000u);
  x[2] = lnd_bits(w.y << 16); x[3] = lnd_bits(w.y & 0xffff0000u);
  x[4] = lnd_bits(w.z << 16); x[5] = lnd_bits(w.z & 0xffff0000u);
  x[6] = lnd_bits(w.w << 16); x[7] = lnd_bits(w.w & 0xffff0000u);
}

// round to nearest even; NaN stays NaN
__device__ __forceinline__ LND_NOPK unsigned int lnd_f2bf(float f) {
  unsigned int u = __builtin_bit_cast(unsigned int, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}

__device__ __forceinline__ LND_NOPK unsigned int lnd_pack2(float lo,
                                                           float hi) {
  return lnd_f2bf(lo) | (lnd_f2bf(hi) << 16);
}

// what __syncthreads() is made of
__device__ __forceinline__ LND_NOPK void lnd_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// 8 consecutive fp32 of gamma / beta: a float4 pair where the base is
// 16-byte aligned (vec), scalar loads for a parameter that is a view at an
// odd offset of a flat buffer
__device__ __forceinline__ LND_NOPK void lnd_load8f(const float* p, bool vec,
                                                    float* o) {
  if (vec) {
    float4 a = reinterpret_cast<const float4*>(p)[0];
    float4 b = reinterpret_cast<const float4*>(p)[1];
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
    o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = p[j];
  }
}

__device__ __forceinline__ LND_NOPK uint4 lnd_pack8(const float* x) {
  uint4 w;
  w.x = lnd_pack2(x[0], x[1]);
  w.y = lnd_pack2(x[2], x[3]);
  w.z = lnd_pack2(x[4], x[5]);
  w.w = lnd_pack2(x[6], x[7]);
  return w;
}

__device__ __forceinline__ LND_NOPK float4 lnd_f4(const float* x) {
  float4 w;
  w.x = x[0]; w.y = x[1]; w.z = x[2]; w.w = x[3];
  return w;
}

// sums of a and b over the G lanes of a row group, in every lane. lds: 8
// floats that no thread of the block still reads from an earlier call.
template <int G>
__device__ __forceinline__ LND_NOPK void lnd_group_sum2(float& a, float& b,
                                                        float* lds) {
  a = ln_wave_sum(a);
  b = ln_wave_sum(b);
  if constexpr (G > 64) {
    constexpr int WPG = G / 64;
    int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
      lds[w] = a;
      lds[4 + w] = b;
    }
    lnd_barrier();
    int w0 = w & ~(WPG - 1);
    a = lds[w0];
    b = lds[4 + w0];
#pragma unroll
    for (int i = 1; i < WPG; ++i) {
      a += lds[w0 + i];
      b += lds[4 + w0 + i];
    }
  }
}

template <int G, int V>
__global__ void
__launch_bounds__(256) LND_NOPK
ln_drop_fwd_kernel(const __hip_bfloat16* __restrict__ x,
                   const __hip_bfloat16* __restrict__ res,  // nullable
                   const float* __restrict__ gamma,
                   const float* __restrict__ beta,
                   __hip_bfloat16* __restrict__ y,
                   __hip_bfloat16* __restrict__ u_out,
                   float* __restrict__ mean_out, float* __restrict__ rstd_out,
                   long N, int H, float eps, float p_drop,
                   unsigned int seed, bool gvec) {
  __shared__ float lds[8];
  const int gl = threadIdx.x & (G - 1);
  const long row = (long)blockIdx.x * (256 / G) + threadIdx.x / G;
  const bool rlive = row < N;
  const int H8 = H >> 3;
  const unsigned int thresh = drop_thresh(p_drop);
  const float rk = p_drop > 0.0f ? 1.0f / (1.0f - p_drop) : 1.0f;
  const long base = row * (long)H8;  // in 16-byte vectors
  const uint4* xv = reinterpret_cast<const uint4*>(x);
  const uint4* rv = reinterpret_cast<const uint4*>(res);
  float v[V][8];
  float acc = 0.f, acc2 = 0.f;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    int c = gl + k * G;
    if (rlive && c < H8) {
      float t[8], r[8];
      lnd_unpack8(xv[base + c], t);
      if (rv) {
        lnd_unpack8(rv[base + c], r);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        bool keep = drop_hash(seed, 0u, (unsigned int)row,
                              (unsigned int)(c * 8 + j)) >= thresh;
        v[k][j] = (keep ? t[j] * rk : 0.f) + r[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[k][j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc += v[k][j];
      acc2 += v[k][j] * v[k][j];
    }
  }
  lnd_group_sum2<G>(acc, acc2, lds);
  float mean = acc / H;
  float var = fmaxf(acc2 / H - mean * mean, 0.f);
  float rstd = rsqrtf(var + eps);
  if (gl == 0 && rlive) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
  uint4* yv = reinterpret_cast<uint4*>(y);
  uint4* uv = reinterpret_cast<uint4*>(u_out);
#pragma unroll
  for (int k = 0; k < V; ++k) {
    int c = gl + k * G;
    if (rlive && c < H8) {
      float gg[8], bt[8], o[8];
      lnd_load8f(gamma + c * 8, gvec, gg);
      lnd_load8f(beta + c * 8, gvec, bt);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[j] = (v[k][j] - mean) * rstd * gg[j] + bt[j];
      yv[base + c] = lnd_pack8(o);
      uv[base + c] = lnd_pack8(v[k]);
    }
  }
}

// partials [gridDim.x, 2, H] fp32: [b, 0] = sum dy * xhat, [b, 1] = sum dy
// over the rows block b walked.
template <int G, int V>
__global__ void
__launch_bounds__(256) LND_NOPK
ln_drop_bwd_kernel(const __hip_bfloat16* __restrict__ dy,
                   const __hip_bfloat16* __restrict__ u,
                   const float* __restrict__ gamma,
                   const float* __restrict__ mean_in,
                   const float* __restrict__ rstd_in,
                   __hip_bfloat16* __restrict__ dx,
                   __hip_bfloat16* __restrict__ dres,
                   float* __restrict__ partials, long N, int H, float p_drop,
                   unsigned int seed, bool gvec) {
  constexpr int RPB = 256 / G;
  static_assert(RPB == 1 || V == 1, "row groups fold one vector per lane");
  __shared__ float red[2][8];
  __shared__ float fold[RPB > 1 ? (RPB - 1) * 2 * 8 * G : 1];
  const int gl = threadIdx.x & (G - 1);
  const int grp = threadIdx.x / G;
  const int H8 = H >> 3;
  const long nrb = (N + RPB - 1) / RPB;
  const unsigned int thresh = drop_thresh(p_drop);
  const float rk = p_drop > 0.0f ? 1.0f / (1.0f - p_drop) : 1.0f;
  const uint4* dyv = reinterpret_cast<const uint4*>(dy);
  const uint4* uv = reinterpret_cast<const uint4*>(u);
  uint4* dxv = reinterpret_cast<uint4*>(dx);
  uint4* drv = reinterpret_cast<uint4*>(dres);

  float gam[V][8], sg[V][8], sb[V][8];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    int c = gl + k * G;
#pragma unroll
    for (int j = 0; j < 8; ++j) gam[k][j] = sg[k][j] = sb[k][j] = 0.f;
    if (c < H8) lnd_load8f(gamma + c * 8, gvec, gam[k]);
  }

  // the next row's loads are issued before the current row is reduced
  uint4 zero4;
  zero4.x = zero4.y = zero4.z = zero4.w = 0u;
  uint4 ndy[V], nu[V];
  float nmean = 0.f, nrstd = 0.f;
  {
    long row = (long)blockIdx.x * RPB + grp;
    bool rl = row < N;
    if (rl) { nmean = mean_in[row]; nrstd = rstd_in[row]; }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      int c = gl + k * G;
      ndy[k] = zero4;
      nu[k] = zero4;
      if (rl && c < H8) {
        ndy[k] = dyv[row * H8 + c];
        nu[k] = uv[row * H8 + c];
      }
    }
  }
  int trip = 0;
  for (long rb = blockIdx.x; rb < nrb; rb += gridDim.x, ++trip) {
    const long row = rb * RPB + grp;
    const bool rlive = row < N;
    uint4 cdy[V], cu[V];
    const float mean = nmean, rstd = nrstd;
#pragma unroll
    for (int k = 0; k < V; ++k) { cdy[k] = ndy[k]; cu[k] = nu[k]; }
    {
      long rbn = rb + gridDim.x;
      long rown = rbn * RPB + grp;
      bool rl = rbn < nrb && rown < N;
      nmean = 0.f; nrstd = 0.f;
      if (rl) { nmean = mean_in[rown]; nrstd = rstd_in[rown]; }
#pragma unroll
      for (int k = 0; k < V; ++k) {
        int c = gl + k * G;
        ndy[k] = zero4;
        nu[k] = zero4;
        if (rl && c < H8) {
          ndy[k] = dyv[rown * H8 + c];
          nu[k] = uv[rown * H8 + c];
        }
      }
    }
    // dead lanes and rows carry dy = 0: they add nothing to any sum
    float d[V][8], xh[V][8];
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      lnd_unpack8(cdy[k], d[k]);
      lnd_unpack8(cu[k], xh[k]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        xh[k][j] = (xh[k][j] - mean) * rstd;
        float g = d[k][j] * gam[k][j];
        c1 += g;
        c2 += g * xh[k][j];
      }
    }
    lnd_group_sum2<G>(c1, c2, red[trip & 1]);
    c1 /= H;
    c2 /= H;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      int c = gl + k * G;
      float o[8], ox[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float dU = rstd * (d[k][j] * gam[k][j] - c1 - xh[k][j] * c2);
        bool keep = drop_hash(seed, 0u, (unsigned int)row,
                              (unsigned int)(c * 8 + j)) >= thresh;
        o[j] = dU;
        ox[j] = keep ? dU * rk : 0.f;
        sb[k][j] += d[k][j];
        sg[k][j] += d[k][j] * xh[k][j];
      }
      if (rlive && c < H8) {
        drv[row * H8 + c] = lnd_pack8(o);
        dxv[row * H8 + c] = lnd_pack8(ox);
      }
    }
  }

  if constexpr (RPB > 1) {
    if (grp > 0) {
      float* f = fold + (grp - 1) * 2 * 8 * G + gl;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        f[j * G] = sg[0][j];
        f[(8 + j) * G] = sb[0][j];
      }
    }
    lnd_barrier();
    if (grp == 0) {
#pragma unroll
      for (int r = 1; r < RPB; ++r) {
        const float* f = fold + (r - 1) * 2 * 8 * G + gl;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          sg[0][j] += f[j * G];
          sb[0][j] += f[(8 + j) * G];
        }
      }
    }
  }
  if (grp == 0) {
    float4* pg = reinterpret_cast<float4*>(partials + (long)blockIdx.x * 2 * H);
    float4* pb = reinterpret_cast<float4*>(partials +
                                           ((long)blockIdx.x * 2 + 1) * H);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      int c = gl + k * G;
      if (c < H8) {
        pg[2 * c] = lnd_f4(sg[k]);
        pg[2 * c + 1] = lnd_f4(sg[k] + 4);
        pb[2 * c] = lnd_f4(sb[k]);
        pb[2 * c + 1] = lnd_f4(sb[k] + 4);
      }
    }
  }
}

// out [2 * H] = sum over b of partials [nb, 2 * H] in a fixed order: a block
// owns LND_FIN_COLS columns; each of its LND_FIN_SLICES slices adds a
// contiguous range of partial rows, ascending, LND_FIN_U rows in flight, and
// slice 0 adds the slice sums in slice order. (One thread a column over all
// nb rows was a chain of nb / LND_FIN_U dependent loads; not measured alone.)
__global__ void
__launch_bounds__(LND_FIN_COLS * LND_FIN_SLICES) LND_NOPK
ln_drop_gb_finalize_kernel(const float* __restrict__ partials,
                           float* __restrict__ out, int nb, int H2) {
  __shared__ float fs[LND_FIN_SLICES][LND_FIN_COLS];
  const int cl = threadIdx.x % LND_FIN_COLS, sl = threadIdx.x / LND_FIN_COLS;
  const int i = blockIdx.x * LND_FIN_COLS + cl;
  const int per = (nb + LND_FIN_SLICES - 1) / LND_FIN_SLICES;
  int b = sl * per;
  const int b1 = b + per < nb ? b + per : nb;
  float s = 0.f;
  if (i < H2) {
    const float* p = partials + i;
    for (; b + LND_FIN_U <= b1; b += LND_FIN_U) {
      float t[LND_FIN_U];
#pragma unroll
      for (int q = 0; q < LND_FIN_U; ++q) t[q] = p[(long)(b + q) * H2];
#pragma unroll
      for (int q = 0; q < LND_FIN_U; ++q) s += t[q];
    }
    for (; b < b1; ++b) s += p[(long)b * H2];
  }
  fs[sl][cl] = s;
  lnd_barrier();
  if (sl == 0 && i < H2) {
#pragma unroll
    for (int q = 1; q < LND_FIN_SLICES; ++q) s += fs[q][cl];
    out[i] = s;
  }
}
