// Fused linear + cross-entropy with an ignore index on gfx950 bf16 matrix
// cores: the BERT masked-LM head loss.
//
//   z[m, v] = Hc[m] . W[v] + b[v]           for the labelled rows only
//   loss[m] = logsumexp_v z[m, v] - z[m, t_m]
//
// The labelled rows are compacted first, so the GEMM runs on count rows and
// not on all N, and the [count, V] logits are never stored: each tile of z
// lives in the MFMA accumulators, is folded into an online log-sum-exp and
// is dropped. Backward recomputes the tiles.
//
// Kernels (256 threads = 4 waves, fp32 accumulation, no atomics anywhere, so
// every output has the same bits run to run):
//
//   lce_scan     one workgroup ranks the labelled rows (label != ignore) in
//                input order: each thread counts a contiguous segment of the
//                labels, an LDS scan turns the counts into bases, a second
//                walk writes rows[rank] (source row) and tgt[rank]. Ranks at
//                or past M_cap are dropped; rows / tgt past the kept ones
//                are -1; count (device memory) is the number kept. Nothing
//                here or later reads count on the host.
//   lce_gather   Hc [M_cap, K] bf16 = h[rows], 16 B per lane, zero pad rows.
//   lce_fwd      grid (row blocks of 64 of Hc, column splits of
//                LCE_SPLIT_COLS). A block whose rows start at or past count
//                returns at once. A wave owns 16 rows x 64 columns of z in
//                the MFMA C layout (col = lane & 15, row = 4 (lane >> 4) +
//                reg). K (up to 1024) is too long for the A fragments to
//                stay in registers, so BOTH operands stream through LDS in
//                chunks of 64 k, double-buffered: the next chunk's global
//                loads (A and W) are issued before the current chunk's
//                MFMAs and stored to the other buffer after them, one block
//                barrier per chunk. Rows of W at or past V are never read
//                (zero fragments). Epilogue in registers: + b[v], ragged
//                columns >= V to the -1e30 sentinel, the target logit picked
//                by the one lane that holds it, online (max, sum exp2) in
//                the log2 domain with dpp16_max / dpp16_sum. Output:
//                partials [splits, M_cap, 2] and z_t [M_cap].
//   lce_combine  one thread per row merges the partials in split order into
//                lse2 (log2 domain) and the row loss, scatters the loss to
//                loss[rows[m]] and tree-adds the block's 256 losses;
//                lce_mean adds the block sums in a fixed tree and divides by
//                count (0 / 0 = NaN with nothing labelled, as
//                F.cross_entropy gives).
//   lce_bwd      the forward's tiling and GEMM body; per tile
//                dz = (exp2(z2 - lse2) - [v == t]) g_row as bf16
//                [M_cap, V_ld] (V_ld = V rounded up to 8; pad columns and
//                rows at or past count zero; blocks past count only write
//                their zeros). g_row = g_rows[rows[m]] + g_mean / count.
//                Column sums of the UNROUNDED dz go wave by wave into LDS
//                and, added in wave order, into partials [row blocks, V_ld].
//   lce_dbias    adds the partials of the live row blocks in block order.
//
// What is NOT here: dHc = dz W and dW = dz^T Hc stay on hipBLASLt through
// torch, and dHc goes back to dh [N, K] by an index_copy on rows
// (ops/fused_linear_ce.py), as the non-fused GEMMs of ssm_ops.hip and
// lstm_ops.hip do.
//
// Packed-fp32 VALU forms are switched off for these kernels, for the reason
// given in ce_ops.hip.
#include "common.h"

#define LCE_NOPK __attribute__((target("no-packed-fp32-ops")))
#define LCE_LN2 0.6931471805599453f
#define LCE_NEG (-1e30f)

typedef short lce_bf16x8 __attribute__((ext_vector_type(8)));
typedef float lce_f32x4 __attribute__((ext_vector_type(4)));

constexpr int LCE_BM = 64;            // rows of Hc per workgroup, 16 per wave
constexpr int LCE_BN = 64;            // vocabulary columns per tile
constexpr int LCE_KC = 64;            // k per LDS chunk: 2 MFMA k-steps
constexpr int LCE_MAX_K = 1024;
constexpr int LCE_PAD = 8;            // LDS row padding (shorts)
constexpr int LCE_ROW = LCE_KC + LCE_PAD;
constexpr int LCE_SPLIT_TILES = 8;    // column tiles walked by one block
constexpr int LCE_SPLIT_COLS = LCE_SPLIT_TILES * LCE_BN;

// round to nearest even; NaN stays NaN
__device__ __forceinline__ LCE_NOPK short lce_f2bf(float f) {
  unsigned u = __builtin_bit_cast(unsigned, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (short)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (short)(u >> 16);
}

// z * log2(e), rounded: a product contracted into a following subtraction
// would differ from the rounded one that went into lse2
__device__ __forceinline__ LCE_NOPK float lce_log2_domain(float z) {
#pragma clang fp contract(off)
  return z * ATTN_LOG2E;
}

// ------------------------------------------------------------------ compact
__global__ void LCE_NOPK __launch_bounds__(256)
lce_scan_kernel(const long* __restrict__ labels, long ignore, int N,
                int M_cap, long* __restrict__ rows, int* __restrict__ tgt,
                int* __restrict__ count) {
  __shared__ int sc[256];
  const int t = threadIdx.x;
  const int per = (N + 255) / 256;
  const int b = min(t * per, N), e = min(b + per, N);
  int c = 0;
  for (int i = b; i < e; ++i) c += labels[i] != ignore;
  sc[t] = c;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int v = t >= off ? sc[t - off] : 0;
    __syncthreads();
    sc[t] += v;
    __syncthreads();
  }
  int rank = sc[t] - c;
  const int kept = min(sc[255], M_cap);
  for (int i = b; i < e; ++i) {
    const long lab = labels[i];
    if (lab != ignore) {
      if (rank < M_cap) {
        rows[rank] = i;
        tgt[rank] = (int)lab;
      }
      ++rank;
    }
  }
  for (int m = kept + t; m < M_cap; m += 256) {
    rows[m] = -1;
    tgt[m] = -1;
  }
  if (t == 0) count[0] = kept;
}

// item idx = (row of Hc, group of 8 columns)
__global__ void LCE_NOPK __launch_bounds__(256)
lce_gather_kernel(const short* __restrict__ h, const long* __restrict__ rows,
                  short* __restrict__ hc, int M_cap, int K) {
  const int c8n = K >> 3;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)M_cap * c8n) return;
  const int m = (int)(idx / c8n), c8 = (int)(idx - (long)m * c8n);
  const long r = rows[m];
  lce_bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (r >= 0) v = *reinterpret_cast<const lce_bf16x8*>(h + r * K + c8 * 8);
  *reinterpret_cast<lce_bf16x8*>(hc + (long)m * K + c8 * 8) = v;
}

// ------------------------------------------------------- forward / backward
// One body for both directions: the z tiles are the same GEMM, only the
// epilogue differs. Unused pointers of the other direction are null.
template <bool BWD>
__device__ __forceinline__ LCE_NOPK void lce_body(
    const short* __restrict__ hc, const short* __restrict__ wt,
    const float* __restrict__ bias, const int* __restrict__ tgt,
    const int* __restrict__ count_p, int M_cap, int V, int V_ld, int K,
    // forward
    float* __restrict__ part, float* __restrict__ zt_out,
    // backward
    const float* __restrict__ lse2, const long* __restrict__ rows,
    const float* __restrict__ g_rows, const float* __restrict__ g_mean,
    short* __restrict__ dz, float* __restrict__ colpart) {
  __shared__ __attribute__((aligned(16))) short As[2 * LCE_BM * LCE_ROW];
  __shared__ __attribute__((aligned(16))) short Bs[2 * LCE_BN * LCE_ROW];
  __shared__ float csum[BWD ? 4 * LCE_SPLIT_COLS : 1];
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int am = l & 15, kg = l >> 4;
  const int count = count_p[0];
  const int rb0 = blockIdx.x * LCE_BM;
  const int tile0 = blockIdx.y * LCE_SPLIT_TILES;
  const int tile1 = min(tile0 + LCE_SPLIT_TILES, (V + LCE_BN - 1) / LCE_BN);

  if (rb0 >= count) {
    // nothing labelled in this row block; backward owes dz its zeros
    if constexpr (BWD) {
      const int c0 = tile0 * LCE_BN;
      const int nvec = (min(tile1 * LCE_BN, V_ld) - c0) >> 3;
      const int nrow = min(LCE_BM, M_cap - rb0);
      const lce_bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int i = t; i < nrow * nvec; i += 256) {
        const int r = i / nvec, c = i - r * nvec;
        *reinterpret_cast<lce_bf16x8*>(dz + (long)(rb0 + r) * V_ld + c0 +
                                       c * 8) = zero;
      }
    }
    return;
  }

  const int nk = K >> 5;
  const int nch = (K + LCE_KC - 1) / LCE_KC;

  // staging: per chunk thread t moves 2 vectors of 8 k of each operand: tile
  // rows (t >> 3) + 32 i at k offset 8 (t & 7); K % 32 == 0, so a vector past
  // K belongs to a k-step that is never multiplied and is skipped. Rows of
  // Hc past M_cap are clamped (nothing is stored for them); rows of W at or
  // past V are not read.
  const int srow = t >> 3, sk = (t & 7) * 8;
  lce_bf16x8 areg[2], wreg[2];
  const short* asrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
    asrc[i] = hc + (long)min(rb0 + srow + 32 * i, M_cap - 1) * K + sk;
#define LCE_LOAD(tile, c)                                                    \
  do {                                                                       \
    if ((c) * LCE_KC + sk < K) {                                             \
      _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                     \
        areg[i_] =                                                           \
            *reinterpret_cast<const lce_bf16x8*>(asrc[i_] + (c) * LCE_KC);   \
        const int v_ = (tile) * LCE_BN + srow + 32 * i_;                     \
        const lce_bf16x8 zero_ = {0, 0, 0, 0, 0, 0, 0, 0};                   \
        wreg[i_] = v_ < V ? *reinterpret_cast<const lce_bf16x8*>(            \
                                wt + (long)v_ * K + (c) * LCE_KC + sk)       \
                          : zero_;                                           \
      }                                                                      \
    }                                                                        \
  } while (0)
#define LCE_STORE(buf, c)                                                    \
  do {                                                                       \
    if ((c) * LCE_KC + sk < K) {                                             \
      const int o_ = ((buf) * LCE_BM + srow) * LCE_ROW + sk;                 \
      _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                     \
        *reinterpret_cast<lce_bf16x8*>(As + o_ + i_ * 32 * LCE_ROW) =        \
            areg[i_];                                                        \
        *reinterpret_cast<lce_bf16x8*>(Bs + o_ + i_ * 32 * LCE_ROW) =        \
            wreg[i_];                                                        \
      }                                                                      \
    }                                                                        \
  } while (0)
  LCE_LOAD(tile0, 0);

  // rows of this lane in the C layout, their targets and row operands
  const int rq = rb0 + w * 16 + kg * 4;
  int tg[4];
  bool rok[4], live[4];
  float ls[4], gg[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    rok[r] = rq + r < M_cap;
    live[r] = rq + r < count;
    const int rc = min(rq + r, M_cap - 1);
    tg[r] = tgt[rc];
    if constexpr (BWD) {
      ls[r] = lse2[rc];
      float g = 0.f;
      if (live[r]) {
        if (g_rows) g = g_rows[rows[rc]];
        if (g_mean) g += g_mean[0] / (float)count;
      }
      gg[r] = g;
    }
  }

  float m_run[4] = {LCE_NEG, LCE_NEG, LCE_NEG, LCE_NEG};
  float s_run[4] = {0.f, 0.f, 0.f, 0.f};

  LCE_STORE(0, 0);
  int cur = 0;
  for (int tile = tile0; tile < tile1; ++tile) {
    lce_f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f},
                        {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int c = 0; c < nch; ++c) {
      __syncthreads();  // buffer cur staged; reads of cur ^ 1 done
      const bool more_k = c + 1 < nch;
      const bool has_next = more_k || tile + 1 < tile1;
      const int ntile = more_k ? tile : tile + 1, nc = more_k ? c + 1 : 0;
      if (has_next) LCE_LOAD(ntile, nc);
      const short* ab =
          As + (cur * LCE_BM + w * 16 + am) * LCE_ROW + kg * 8;
      const short* bb = Bs + (cur * LCE_BN + am) * LCE_ROW + kg * 8;
#pragma unroll
      for (int j = 0; j < LCE_KC / 32; ++j) {
        if (c * (LCE_KC / 32) + j < nk) {
          const lce_bf16x8 af =
              *reinterpret_cast<const lce_bf16x8*>(ab + j * 32);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const lce_bf16x8 bf = *reinterpret_cast<const lce_bf16x8*>(
                bb + q * 16 * LCE_ROW + j * 32);
            acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[q],
                                                             0, 0, 0);
          }
        }
      }
      if (has_next) LCE_STORE(cur ^ 1, nc);
      cur ^= 1;
    }

    // epilogue operands of this lane's four columns
    bool cok[4];
    float bv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int s = tile * LCE_BN + q * 16 + am;
      cok[q] = s < V;
      bv[q] = (bias && cok[q]) ? bias[s] : 0.f;
    }

    if constexpr (!BWD) {
      float v[4][4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int s = tile * LCE_BN + q * 16 + am;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float z = acc[q][r] + bv[q];
          v[q][r] = cok[q] ? lce_log2_domain(z) : LCE_NEG;
          if (cok[q] && s == tg[r] && rok[r]) zt_out[rq + r] = z;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float tm = fmaxf(fmaxf(v[0][r], v[1][r]), fmaxf(v[2][r], v[3][r]));
        const float mn = fmaxf(m_run[r], dpp16_max(tm));
        float ps = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          ps += v[q][r] > 0.5f * LCE_NEG ? exp2f(v[q][r] - mn) : 0.f;
        s_run[r] = s_run[r] * exp2f(m_run[r] - mn) + dpp16_sum(ps);
        m_run[r] = mn;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int s = tile * LCE_BN + q * 16 + am;
        float cs = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = exp2f(lce_log2_domain(acc[q][r] + bv[q]) - ls[r]);
          const float d = (cok[q] && live[r])
                              ? (p - (s == tg[r] ? 1.0f : 0.0f)) * gg[r]
                              : 0.f;
          cs += d;
          if (rok[r] && s < V_ld) dz[(long)(rq + r) * V_ld + s] = lce_f2bf(d);
        }
        cs += __shfl_xor(cs, 16, 64);
        cs += __shfl_xor(cs, 32, 64);
        if (kg == 0) csum[w * LCE_SPLIT_COLS + s - tile0 * LCE_BN] = cs;
      }
    }
  }
#undef LCE_LOAD
#undef LCE_STORE

  if constexpr (!BWD) {
    if (am == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (rok[r]) {
          float* p = part + ((long)blockIdx.y * M_cap + rq + r) * 2;
          p[0] = m_run[r];
          p[1] = s_run[r];
        }
      }
    }
  } else {
    __syncthreads();
    if (colpart) {
      const int ncols = min(tile1 * LCE_BN, V_ld) - tile0 * LCE_BN;
      for (int c = t; c < ncols; c += 256)
        colpart[(long)blockIdx.x * V_ld + tile0 * LCE_BN + c] =
            ((csum[c] + csum[LCE_SPLIT_COLS + c]) +
             csum[2 * LCE_SPLIT_COLS + c]) +
            csum[3 * LCE_SPLIT_COLS + c];
    }
  }
}

__global__ void LCE_NOPK __launch_bounds__(256)
lce_fwd_kernel(const short* __restrict__ hc, const short* __restrict__ wt,
               const float* __restrict__ bias, const int* __restrict__ tgt,
               const int* __restrict__ count, float* __restrict__ part,
               float* __restrict__ zt, int M_cap, int V, int K) {
  lce_body<false>(hc, wt, bias, tgt, count, M_cap, V, 0, K, part, zt, nullptr,
                  nullptr, nullptr, nullptr, nullptr, nullptr);
}

__global__ void LCE_NOPK __launch_bounds__(256)
lce_bwd_kernel(const short* __restrict__ hc, const short* __restrict__ wt,
               const float* __restrict__ bias, const int* __restrict__ tgt,
               const int* __restrict__ count, const float* __restrict__ lse2,
               const long* __restrict__ rows, const float* __restrict__ g_rows,
               const float* __restrict__ g_mean, short* __restrict__ dz,
               float* __restrict__ colpart, int M_cap, int V, int V_ld,
               int K) {
  lce_body<true>(hc, wt, bias, tgt, count, M_cap, V, V_ld, K, nullptr,
                 nullptr, lse2, rows, g_rows, g_mean, dz, colpart);
}

// One thread per row of Hc: the partials [splits, M_cap, 2] in split order.
// Rows at or past count get lse2 = 0 and add 0 to the block's sum, so the
// sums do not depend on M_cap. loss_n [N] arrives zeroed.
__global__ void LCE_NOPK __launch_bounds__(256)
lce_combine_kernel(const float* __restrict__ part, const float* __restrict__ zt,
                   const long* __restrict__ rows, const int* __restrict__ count,
                   float* __restrict__ loss_n, float* __restrict__ lse2,
                   float* __restrict__ blocksum, int M_cap, int splits) {
  __shared__ float red[256];
  const int t = threadIdx.x, m = blockIdx.x * 256 + t;
  float loss = 0.f;
  if (m < M_cap) {
    float l2e = 0.f;
    if (m < count[0]) {
      const float z2 = lce_log2_domain(zt[m]);
      float M = LCE_NEG;
      for (int k = 0; k < splits; ++k)
        M = fmaxf(M, part[((long)k * M_cap + m) * 2]);
      float sum = 0.f;
      for (int k = 0; k < splits; ++k) {
        const float* p = part + ((long)k * M_cap + m) * 2;
        sum += p[1] * exp2f(p[0] - M);
      }
      const float l2 = log2f(sum);
      l2e = M + l2;
      loss = ((M - z2) + l2) * LCE_LN2;
      loss_n[rows[m]] = loss;
    }
    lse2[m] = l2e;
  }
  red[t] = loss;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) red[t] += red[t + off];
    __syncthreads();
  }
  if (t == 0) blocksum[blockIdx.x] = red[0];
}

// out[0] = sum of the block sums (fixed tree), out[1] = out[0] / count
__global__ void LCE_NOPK __launch_bounds__(256)
lce_mean_kernel(const float* __restrict__ blocksum,
                const int* __restrict__ count, float* __restrict__ out,
                int nblocks) {
  __shared__ float red[256];
  const int t = threadIdx.x;
  float a = 0.f;
  for (int b = t; b < nblocks; b += 256) a += blocksum[b];
  red[t] = a;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) red[t] += red[t + off];
    __syncthreads();
  }
  if (t == 0) {
    out[0] = red[0];
    out[1] = red[0] / (float)count[0];
  }
}

// db[v] = sum over the live row blocks, in block order
__global__ void LCE_NOPK __launch_bounds__(256)
lce_dbias_kernel(const float* __restrict__ colpart,
                 const int* __restrict__ count, float* __restrict__ db, int V,
                 int V_ld, int row_blocks) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const int nb = min(row_blocks, (count[0] + LCE_BM - 1) / LCE_BM);
  float a = 0.f;
  for (int b = 0; b < nb; ++b) a += colpart[(long)b * V_ld + v];
  db[v] = a;
}
