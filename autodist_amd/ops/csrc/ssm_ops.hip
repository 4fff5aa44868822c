// Sampled softmax loss (TF's sampled_softmax_loss with remove_accidental_hits
// and subtract_log_q) on gfx950 bf16 matrix cores: the LM1B training loss.
//
//   z0[n]   = h[n] . W[t_n] + b[t_n] - logq_true[n]
//   z[n,s]  = h[n] . W[c_s] + b[c_s] - logq_samp[s],  removed where c_s == t_n
//   loss[n] = logsumexp(z0[n], z[n, 0..S)) - z0[n]
//
// Kernels (256 threads = 4 waves, fp32 accumulation, no atomics anywhere, so
// every output has the same bits run to run):
//
//   ssm_prep     one pass over the S + N table rows the loss touches: gathers
//                W[c_s] into Wg [S_pad, P] and W[t_n] into Wt [N, P], both
//                bf16 (the cast from an fp32 table happens here, on S + N rows
//                and not on the whole table), 16 B per lane, P / 8 consecutive
//                lanes per row; off[s] = b[c_s] - logq_samp[s] and off0[n] =
//                b[t_n] - logq_true[n]. Pad rows of Wg (S_pad = S rounded up
//                to the column tile) are zero.
//   ssm_fwd      grid (row blocks of 64, column splits of SSM_SPLIT_COLS). A
//                wave owns 16 rows of h and keeps their A fragments for the
//                whole K = P in registers (P / 32 fragments, at most 16: 64
//                VGPRs). Wg streams through LDS in chunks of 64 columns x 128
//                k, double-buffered and shared by the four waves: the next
//                chunk's global loads are issued before the current chunk's
//                MFMAs and stored to the other buffer after them, one block
//                barrier per chunk. B fragments are ds_read_b128. Per column
//                tile the wave holds a 16 x 64 block of z in the MFMA C layout
//                (col = lane & 15, row = 4 (lane >> 4) + reg) and runs the
//                epilogue in registers: + off[s], removed / pad / ragged
//                columns to the -1e30 sentinel, online (max, sum exp2) in the
//                log2 domain with dpp16_max / dpp16_sum. Output: partial
//                statistics [splits, N, 2]. Blocks of split 0 also form z0[n]
//                from the resident A fragments and Wt[n].
//   ssm_combine  one thread per row merges z0 and the partials in split order:
//                loss[n], lse2[n] (log2 domain).
//   ssm_bwd      the forward's tiling; recomputes each z tile on MFMA and
//                stores dz = exp2(z2 - lse2) g as bf16 [N, S_pad] (zeros in
//                removed and pad columns). Column sums of the UNROUNDED dz go
//                wave by wave into LDS and, added in wave order, into
//                partials [row blocks, S_pad]; ssm_dbias adds those in block
//                order. Blocks of split 0 write dz0[n].
//
// What is NOT here: dH = dz Wg, dWg = dz^T H and the row-wise dz0 terms stay
// on hipBLASLt / torch (ops/sampled_softmax.py), as the non-recurrent GEMMs
// of lstm_ops.hip do.
//
// Packed-fp32 VALU forms are switched off for these kernels, for the reason
// given in ce_ops.hip.
#include "common.h"

#define SSM_NOPK __attribute__((target("no-packed-fp32-ops")))
#define SSM_LN2 0.6931471805599453f
#define SSM_NEG (-1e30f)

typedef short ssm_bf16x8 __attribute__((ext_vector_type(8)));
typedef float ssm_f32x4 __attribute__((ext_vector_type(4)));

constexpr int SSM_BM = 64;            // rows of h per workgroup, 16 per wave
constexpr int SSM_BN = 64;            // candidate columns per LDS tile
constexpr int SSM_CHUNK_STEPS = 4;    // MFMA k-steps (of 32) per chunk
constexpr int SSM_KC = 32 * SSM_CHUNK_STEPS;
constexpr int SSM_MAX_CHUNKS = 4;     // chunks per column tile at most
constexpr int SSM_MAX_KSTEPS = SSM_CHUNK_STEPS * SSM_MAX_CHUNKS;
constexpr int SSM_MAX_P = 32 * SSM_MAX_KSTEPS;   // A fragments in registers
constexpr int SSM_PAD = 8;            // LDS row padding (shorts)
constexpr int SSM_WROW = SSM_KC + SSM_PAD;
constexpr int SSM_SPLIT_TILES = 8;    // column tiles walked by one block
constexpr int SSM_SPLIT_COLS = SSM_SPLIT_TILES * SSM_BN;

__device__ __forceinline__ SSM_NOPK float ssm_bf2f(short s) {
  return __builtin_bit_cast(float, ((unsigned)(unsigned short)s) << 16);
}

// round to nearest even; NaN stays NaN
__device__ __forceinline__ SSM_NOPK short ssm_f2bf(float f) {
  unsigned u = __builtin_bit_cast(unsigned, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (short)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (short)(u >> 16);
}

// z0 * log2(e), rounded: a product contracted into a following subtraction
// would not cancel against the rounded one kept in lse2
__device__ __forceinline__ SSM_NOPK float ssm_log2_domain(float z) {
#pragma clang fp contract(off)
  return z * ATTN_LOG2E;
}

__device__ __forceinline__ SSM_NOPK ssm_bf16x8 ssm_load8(const float* p) {
  float4 a = *reinterpret_cast<const float4*>(p);
  float4 b = *reinterpret_cast<const float4*>(p + 4);
  ssm_bf16x8 r = {ssm_f2bf(a.x), ssm_f2bf(a.y), ssm_f2bf(a.z), ssm_f2bf(a.w),
                  ssm_f2bf(b.x), ssm_f2bf(b.y), ssm_f2bf(b.z), ssm_f2bf(b.w)};
  return r;
}

__device__ __forceinline__ SSM_NOPK ssm_bf16x8 ssm_load8(const short* p) {
  return *reinterpret_cast<const ssm_bf16x8*>(p);
}

// --------------------------------------------------------------------- prep
// Item idx = (row, group of 8 columns); rows [0, S_pad) are Wg, rows
// [S_pad, S_pad + N) are Wt. T is the table's element type (float or bf16
// bits).
template <typename T>
__global__ void SSM_NOPK __launch_bounds__(256)
ssm_prep_kernel(const T* __restrict__ table, const float* __restrict__ bias,
                const long* __restrict__ cand, const long* __restrict__ tgt,
                const float* __restrict__ logq_samp,
                const float* __restrict__ logq_true, short* __restrict__ wg,
                short* __restrict__ wt, float* __restrict__ off,
                float* __restrict__ off0, int S, int S_pad, int N, int P) {
  const int c8n = P >> 3;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= ((long)S_pad + N) * c8n) return;
  const int row = (int)(idx / c8n), c8 = (int)(idx - (long)row * c8n);
  const bool is_t = row >= S_pad;
  const int n = row - S_pad;
  short* dst = (is_t ? wt + (long)n * P : wg + (long)row * P) + c8 * 8;
  if (!is_t && row >= S) {
    const ssm_bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    *reinterpret_cast<ssm_bf16x8*>(dst) = zero;
    if (c8 == 0) off[row] = 0.f;
    return;
  }
  const long id = is_t ? tgt[n] : cand[row];
  *reinterpret_cast<ssm_bf16x8*>(dst) = ssm_load8(table + id * P + c8 * 8);
  if (c8 == 0) {
    float b = bias ? bias[id] : 0.f;
    if (is_t)
      off0[n] = b - logq_true[n];
    else
      off[row] = b - logq_samp[row];
  }
}

// ------------------------------------------------------- forward / backward
// One body for both directions: the z tiles are the same GEMM, only the
// epilogue differs. Unused pointers of the other direction are null.
template <bool BWD>
__device__ __forceinline__ SSM_NOPK void ssm_body(
    const short* __restrict__ h, const short* __restrict__ wg,
    const float* __restrict__ off, const long* __restrict__ cand,
    const long* __restrict__ tgt, int N, int S, int S_pad, int P,
    // forward
    const short* __restrict__ wt, const float* __restrict__ off0,
    float* __restrict__ part, float* __restrict__ z0_out,
    // backward
    const float* __restrict__ lse2, const float* __restrict__ z0_in,
    const float* __restrict__ g, short* __restrict__ dz,
    float* __restrict__ colpart, float* __restrict__ dz0_out) {
  __shared__ __attribute__((aligned(16))) short Ws[2 * SSM_BN * SSM_WROW];
  __shared__ float csum[BWD ? 4 * SSM_SPLIT_COLS : 1];
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int am = l & 15, kg = l >> 4;
  const int r0 = blockIdx.x * SSM_BM + w * 16;
  const int nk = P >> 5;
  const int tile0 = blockIdx.y * SSM_SPLIT_TILES;
  const int tile1 = min(tile0 + SSM_SPLIT_TILES, S_pad / SSM_BN);

  // B staging: per chunk thread t moves 4 vectors of 8 k: tile rows
  // (t >> 4) + 16 i at k offset 8 (t & 15); P % 32 == 0, so a vector past P
  // belongs to a k-step that is never multiplied and is skipped
  const int srow = t >> 4, sk = (t & 15) * 8;
  ssm_bf16x8 wreg[4];
#define SSM_LOAD_W(tile, c)                                                  \
  do {                                                                       \
    if ((c) * SSM_KC + sk < P) {                                             \
      const short* src_ =                                                    \
          wg + ((long)(tile) * SSM_BN + srow) * P + (c) * SSM_KC + sk;       \
      _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) wreg[i_] =            \
          *reinterpret_cast<const ssm_bf16x8*>(src_ + (long)i_ * 16 * P);    \
    }                                                                        \
  } while (0)
#define SSM_STORE_W(buf, c)                                                  \
  do {                                                                       \
    if ((c) * SSM_KC + sk < P) {                                             \
      short* dst_ = Ws + ((buf) * SSM_BN + srow) * SSM_WROW + sk;            \
      _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                       \
          *reinterpret_cast<ssm_bf16x8*>(dst_ + i_ * 16 * SSM_WROW) =        \
          wreg[i_];                                                          \
    }                                                                        \
  } while (0)
  SSM_LOAD_W(tile0, 0);

  // A fragments of this wave's 16 rows for the whole K (rows past N clamped;
  // nothing is stored for them)
  ssm_bf16x8 af[SSM_MAX_KSTEPS];
  {
    const short* hrow = h + (long)min(r0 + am, N - 1) * P + kg * 8;
#pragma unroll
    for (int kc = 0; kc < SSM_MAX_KSTEPS; ++kc) {
      const ssm_bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
      af[kc] = kc < nk ? *reinterpret_cast<const ssm_bf16x8*>(hrow + kc * 32)
                       : zero;
    }
  }

  // rows of this lane in the C layout, their targets and row operands
  const int rq = r0 + kg * 4;
  int tg[4];
  bool rok[4];
  float ls[4], gg[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    rok[r] = rq + r < N;
    const int rc = min(rq + r, N - 1);
    tg[r] = (int)tgt[rc];
    if constexpr (BWD) {
      ls[r] = lse2[rc];
      gg[r] = g[rc];
    }
  }

  if (blockIdx.y == 0) {
    const int row = r0 + am;
    if constexpr (BWD) {
      if (kg == 0 && row < N)
        dz0_out[row] =
            (exp2f(ssm_log2_domain(z0_in[row]) - lse2[row]) - 1.0f) * g[row];
    } else {
      // z0: row-wise dot of the resident A fragments with Wt
      const short* wrow = wt + (long)min(row, N - 1) * P + kg * 8;
      float d = 0.f;
#pragma unroll
      for (int kc = 0; kc < SSM_MAX_KSTEPS; ++kc) {
        if (kc < nk) {
          ssm_bf16x8 wv = *reinterpret_cast<const ssm_bf16x8*>(wrow + kc * 32);
#pragma unroll
          for (int e = 0; e < 8; ++e)
            d = fmaf(ssm_bf2f(af[kc][e]), ssm_bf2f(wv[e]), d);
        }
      }
      d += __shfl_xor(d, 16, 64);
      d += __shfl_xor(d, 32, 64);
      if (kg == 0 && row < N) z0_out[row] = d + off0[row];
    }
  }

  float m_run[4] = {SSM_NEG, SSM_NEG, SSM_NEG, SSM_NEG};
  float s_run[4] = {0.f, 0.f, 0.f, 0.f};

  SSM_STORE_W(0, 0);
  int cur = 0;
  for (int tile = tile0; tile < tile1; ++tile) {
    // epilogue operands of this lane's four columns; a pad column has id -1
    int cid[4];
    float offv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int s = tile * SSM_BN + q * 16 + am;
      cid[q] = s < S ? (int)cand[s] : -1;
      offv[q] = off[s];
    }
    ssm_f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f},
                        {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int c = 0; c < SSM_MAX_CHUNKS; ++c) {
      if (c * SSM_CHUNK_STEPS < nk) {
        __syncthreads();  // buffer cur staged; reads of cur ^ 1 done
        const bool more_k = (c + 1) * SSM_CHUNK_STEPS < nk;
        const bool has_next = more_k || tile + 1 < tile1;
        if (has_next) {
          if (more_k)
            SSM_LOAD_W(tile, c + 1);
          else
            SSM_LOAD_W(tile + 1, 0);
        }
        const short* wb = Ws + (cur * SSM_BN + am) * SSM_WROW + kg * 8;
#pragma unroll
        for (int j = 0; j < SSM_CHUNK_STEPS; ++j) {
          if (c * SSM_CHUNK_STEPS + j < nk) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              ssm_bf16x8 bf = *reinterpret_cast<const ssm_bf16x8*>(
                  wb + q * 16 * SSM_WROW + j * 32);
              acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  af[c * SSM_CHUNK_STEPS + j], bf, acc[q], 0, 0, 0);
            }
          }
        }
        if (has_next) {
          if (more_k)
            SSM_STORE_W(cur ^ 1, c + 1);
          else
            SSM_STORE_W(cur ^ 1, 0);
        }
        cur ^= 1;
      }
    }

    if constexpr (!BWD) {
      float v[4][4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool rm = cid[q] < 0 || cid[q] == tg[r];
          v[q][r] = rm ? SSM_NEG : (acc[q][r] + offv[q]) * ATTN_LOG2E;
        }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float tm = fmaxf(fmaxf(v[0][r], v[1][r]), fmaxf(v[2][r], v[3][r]));
        const float mn = fmaxf(m_run[r], dpp16_max(tm));
        float ps = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          ps += v[q][r] > 0.5f * SSM_NEG ? exp2f(v[q][r] - mn) : 0.f;
        s_run[r] = s_run[r] * exp2f(m_run[r] - mn) + dpp16_sum(ps);
        m_run[r] = mn;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int s = tile * SSM_BN + q * 16 + am;
        float cs = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool rm = cid[q] < 0 || cid[q] == tg[r] || !rok[r];
          const float d =
              rm ? 0.f
                 : exp2f((acc[q][r] + offv[q]) * ATTN_LOG2E - ls[r]) * gg[r];
          cs += d;
          if (rok[r]) dz[(long)(rq + r) * S_pad + s] = ssm_f2bf(d);
        }
        cs += __shfl_xor(cs, 16, 64);
        cs += __shfl_xor(cs, 32, 64);
        if (kg == 0) csum[w * SSM_SPLIT_COLS + s - tile0 * SSM_BN] = cs;
      }
    }
  }
#undef SSM_LOAD_W
#undef SSM_STORE_W

  if constexpr (!BWD) {
    if (am == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (rok[r]) {
          float* p = part + ((long)blockIdx.y * N + rq + r) * 2;
          p[0] = m_run[r];
          p[1] = s_run[r];
        }
      }
    }
  } else {
    __syncthreads();
    const int ncols = (tile1 - tile0) * SSM_BN;
    for (int c = t; c < ncols; c += 256)
      colpart[(long)blockIdx.x * S_pad + tile0 * SSM_BN + c] =
          ((csum[c] + csum[SSM_SPLIT_COLS + c]) +
           csum[2 * SSM_SPLIT_COLS + c]) +
          csum[3 * SSM_SPLIT_COLS + c];
  }
}

__global__ void SSM_NOPK __launch_bounds__(256)
ssm_fwd_kernel(const short* __restrict__ h, const short* __restrict__ wg,
               const short* __restrict__ wt, const float* __restrict__ off,
               const float* __restrict__ off0, const long* __restrict__ cand,
               const long* __restrict__ tgt, float* __restrict__ part,
               float* __restrict__ z0, int N, int S, int S_pad, int P) {
  ssm_body<false>(h, wg, off, cand, tgt, N, S, S_pad, P, wt, off0, part, z0,
                  nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

__global__ void SSM_NOPK __launch_bounds__(256)
ssm_bwd_kernel(const short* __restrict__ h, const short* __restrict__ wg,
               const float* __restrict__ off, const long* __restrict__ cand,
               const long* __restrict__ tgt, const float* __restrict__ lse2,
               const float* __restrict__ z0, const float* __restrict__ g,
               short* __restrict__ dz, float* __restrict__ colpart,
               float* __restrict__ dz0, int N, int S, int S_pad, int P) {
  ssm_body<true>(h, wg, off, cand, tgt, N, S, S_pad, P, nullptr, nullptr,
                 nullptr, nullptr, lse2, z0, g, dz, colpart, dz0);
}

// one thread per row: z0 and the partials [splits, N, 2] in split order. The
// loss is formed from (M - z0) and log2(sum) separately, so a row whose
// candidates are all removed gets exactly 0 (and, in backward, dz0 == 0).
__global__ void SSM_NOPK __launch_bounds__(256)
ssm_combine_kernel(const float* __restrict__ part, const float* __restrict__ z0,
                   float* __restrict__ loss, float* __restrict__ lse2, int N,
                   int splits) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float z2 = ssm_log2_domain(z0[n]);
  float M = z2;
  for (int k = 0; k < splits; ++k) M = fmaxf(M, part[((long)k * N + n) * 2]);
  float sum = exp2f(z2 - M);
  for (int k = 0; k < splits; ++k) {
    const float* p = part + ((long)k * N + n) * 2;
    sum += p[1] * exp2f(p[0] - M);
  }
  const float l2 = log2f(sum);
  lse2[n] = M + l2;
  loss[n] = ((M - z2) + l2) * SSM_LN2;
}

// db_samp[s] = sum over row blocks, in block order
__global__ void SSM_NOPK __launch_bounds__(256)
ssm_dbias_kernel(const float* __restrict__ colpart, float* __restrict__ db,
                 int S, int S_pad, int row_blocks) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  float a = 0.f;
  for (int b = 0; b < row_blocks; ++b) a += colpart[(long)b * S_pad + s];
  db[s] = a;
}
