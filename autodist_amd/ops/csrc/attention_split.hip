// Split-KV attention FORWARD on gfx950 matrix cores (no dropout).
//
// attn_fwd_kernel (attention.hip) gives one workgroup a whole 64*RB-row query
// block: it walks all S keys alone, so B*H*ceil(S / (64*RB)) workgroups are
// all the parallelism there is. At serving shapes (B = 1..4, S >= 512) that
// is a fraction of the 256 CUs. Here the keys of one (b, h, query block) are
// cut into n contiguous ranges of 64-key tiles, one workgroup each:
//
//   attn_fwd_split_kernel<RB, D>   the forward's tiling on tiles
//       [split * tps, min((split + 1) * tps, T)), T = ceil(S / 64),
//       tps = ceil(T / n). No division, no bf16 store: it writes the
//       UNnormalised fp32 accumulator o_part[split, bh, q, D] and the row
//       statistics m_part / l_part [split, bh, q] (exp2 domain).
//   attn_fwd_combine_kernel<D>     per (bh, q) row: M = max_s m_s,
//       w_s = exp2(m_s - M), L = sum_s l_s w_s, O = (sum_s o_s w_s) / L in
//       ascending split order -> bf16 [B, H, S, D]. No atomics.
//
// Grid of the split kernel: (split * nqb + qb) * NBH + bh. (b, h) stays the
// fast dimension, so every workgroup of one head, its splits included, lands
// on one XCD's L2 when B*H % 8 == 0, as in the one-kernel forward.
//
// The main loop is the forward's, statement for statement (64-key K/V tiles
// in double-buffered LDS, V transposed, P staged bf16 per wave, exp2-domain
// online softmax on dpp16_max / dpp16_sum), minus the dropout hash: with one
// split the accumulator and statistics are the forward's own, w_0 = 1 and
// L = l_0 exactly, and the combine's acc / L is the forward's epilogue, so
// the result is bit-equal to attn_fwd (tests/test_attention_split_gpu.py).
//
// Partial store. The MFMA C layout leaves a lane 4 rows x 1 column per
// d-tile: stored directly that is D/4 scattered 4-byte stores per lane. The
// accumulator instead goes through LDS (the K buffers, free after the last
// tile; conflict-free with the D + 4 float row pitch) and leaves as 16-byte
// stores, 16 or 32 lanes covering one contiguous 256 / 512-byte row.
//
// Included after attention.hip (ext.hip): uses its bf16x8_t / f32x4_t, KPAD
// and wave_lds_fence.
#include "common.h"

#define ATTN_MAX_SPLITS 8
#define ATTN_SPLIT_NOPK __attribute__((target("no-packed-fp32-ops")))

template <int RB, int D>
__global__ void ATTN_SPLIT_NOPK
__launch_bounds__(256, D == 64 ? 2 : 1)
attn_fwd_split_kernel(const __hip_bfloat16* __restrict__ Q,
                      const __hip_bfloat16* __restrict__ K,
                      const __hip_bfloat16* __restrict__ V,
                      float* __restrict__ o_part,   // [n, NBH, S, D]
                      float* __restrict__ m_part,   // [n, NBH, S]
                      float* __restrict__ l_part,   // [n, NBH, S]
                      const float* __restrict__ mask, long S, long H, long NBH,
                      long nqb, long tiles_per_split,
                      long q_sb, long q_sh, long q_ss,
                      long k_sb, long k_sh, long k_ss,
                      long v_sb, long v_sh, long v_ss, float scale) {
  __shared__ __attribute__((aligned(16))) short Ks[2][64][D + KPAD];
  __shared__ short VsT[2][D][64 + KPAD];
  __shared__ short Pw[4][16][64 + KPAD];
  constexpr int OPITCH = D + 4;  // fp32 row pitch of the epilogue staging
  static_assert(4 * 16 * OPITCH * sizeof(float) <= sizeof(Ks),
                "accumulator staging must fit in the K buffers");
  int t = threadIdx.x;
  int w = t >> 6;
  int l = t & 63;
  long bh = (long)blockIdx.x % NBH;
  long rest = (long)blockIdx.x / NBH;
  long qb = rest % nqb;
  long split = rest / nqb;
  long q0 = qb * (64 * RB) + w * (16 * RB);
  long b = bh / H, hh = bh % H;
  const short* q_p = reinterpret_cast<const short*>(Q) + b * q_sb + hh * q_sh;
  const short* k_p = reinterpret_cast<const short*>(K) + b * k_sb + hh * k_sh;
  const short* v_p = reinterpret_cast<const short*>(V) + b * v_sb + hh * v_sh;
  const float* m_p = mask ? mask + b * S : nullptr;
  // this split's keys: whole tiles; the host guarantees k_beg < S
  const long k_beg = split * tiles_per_split * 64;
  const long k_end = k_beg + tiles_per_split * 64 < S
                         ? k_beg + tiles_per_split * 64 : S;

  constexpr int NC = D / 32;
  constexpr int ND = D / 16;
  int am = l & 15;
  int kg = l >> 4;
  const float scale2 = scale * ATTN_LOG2E;

  bf16x8_t qf[RB][NC];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    int qrow_a = q0 + rb * 16 + am < S ? (int)q0 + rb * 16 + am : (int)S - 1;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        qf[rb][c][j] = q_p[qrow_a * q_ss + c * 32 + kg * 8 + j];
      }
    }
  }

  float m_run[RB][4], l_run[RB][4];
  f32x4_t o_acc[RB][ND];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m_run[rb][r] = -1e30f;
      l_run[rb][r] = 0.f;
    }
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) o_acc[rb][dt] = {0.f, 0.f, 0.f, 0.f};
  }

  int srow = t >> 2, scol = (t & 3) * (D / 4);
  constexpr int NH = D / 32;

  bf16x8_t kreg[NH], vreg[NH];
  // the lambdas carry the target attribute too: without it they are not
  // inlined and their captures live in scratch
  auto load_tile = [&](long kt) ATTN_SPLIT_NOPK {
    int krow = kt + srow < S ? (int)kt + srow : (int)S - 1;
#pragma unroll
    for (int half = 0; half < NH; ++half) {
      kreg[half] = *reinterpret_cast<const bf16x8_t*>(
          &k_p[krow * k_ss + scol + half * 8]);
      vreg[half] = *reinterpret_cast<const bf16x8_t*>(
          &v_p[krow * v_ss + scol + half * 8]);
    }
  };
  auto store_tile = [&](int buf) ATTN_SPLIT_NOPK {
#pragma unroll
    for (int half = 0; half < NH; ++half) {
      *reinterpret_cast<bf16x8_t*>(&Ks[buf][srow][scol + half * 8]) =
          kreg[half];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        VsT[buf][scol + half * 8 + j][srow] = vreg[half][j];
    }
  };

  load_tile(k_beg);
  store_tile(0);
  int cur = 0;
  for (long kt = k_beg; kt < k_end; kt += 64) {
    __syncthreads();
    bool has_next = kt + 64 < k_end;
    if (has_next) load_tile(kt + 64);

    float mv2[4], oob[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      int key = (int)kt + h * 16 + am;
      mv2[h] = (m_p && key < (int)S) ? m_p[key] * ATTN_LOG2E : 0.f;
      oob[h] = key < (int)S ? 0.f : -1e30f;
    }

#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      f32x4_t s_acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f},
                          {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int h = 0; h < 4; ++h) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          bf16x8_t kf = *reinterpret_cast<const bf16x8_t*>(
              &Ks[cur][h * 16 + am][c * 32 + kg * 8]);
          s_acc[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              qf[rb][c], kf, s_acc[h], 0, 0, 0);
        }
      }
      float sv[4][4];
#pragma unroll
      for (int h = 0; h < 4; ++h) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          sv[h][r] = s_acc[h][r] * scale2 + mv2[h] + oob[h];
      }
      float alpha[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float smax = fmaxf(fmaxf(sv[0][r], sv[1][r]),
                           fmaxf(sv[2][r], sv[3][r]));
        float tmax = dpp16_max(smax);
        float m_new = fmaxf(m_run[rb][r], tmax);
        alpha[r] = exp2f(m_run[rb][r] - m_new);
        float psum = 0.f;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          sv[h][r] = exp2f(sv[h][r] - m_new);
          psum += sv[h][r];
        }
        l_run[rb][r] = l_run[rb][r] * alpha[r] + dpp16_sum(psum);
        m_run[rb][r] = m_new;
      }
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o_acc[rb][dt][r] *= alpha[r];
      }
#pragma unroll
      for (int h = 0; h < 4; ++h) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          __hip_bfloat16 pb = __float2bfloat16(sv[h][r]);
          Pw[w][kg * 4 + r][h * 16 + am] = reinterpret_cast<short&>(pb);
        }
      }
      wave_lds_fence();
      bf16x8_t pf[2];
#pragma unroll
      for (int kc = 0; kc < 2; ++kc) {
        pf[kc] = *reinterpret_cast<const bf16x8_t*>(
            &Pw[w][am][kc * 32 + kg * 8]);
      }
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) {
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
          bf16x8_t vf = *reinterpret_cast<const bf16x8_t*>(
              &VsT[cur][dt * 16 + am][kc * 32 + kg * 8]);
          o_acc[rb][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              pf[kc], vf, o_acc[rb][dt], 0, 0, 0);
        }
      }
      wave_lds_fence();
    }
    if (has_next) store_tile(1 - cur);
    cur = 1 - cur;
  }

  // ---- epilogue: statistics, then the raw accumulator through LDS
  const long row_base = (split * NBH + bh) * S;  // partial row of q = 0
  if (am == 0) {  // the 16 lanes of a C-column group hold the same m, l
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        long qrow = q0 + rb * 16 + kg * 4 + r;
        if (qrow >= S) continue;
        m_part[row_base + qrow] = m_run[rb][r];
        l_part[row_base + qrow] = l_run[rb][r];
      }
    }
  }
  __syncthreads();  // every wave is done with Ks before it is reused
  float* ow = reinterpret_cast<float*>(&Ks[0][0][0]) + w * (16 * OPITCH);
  constexpr int V4 = D / 4;            // float4s per row
  constexpr int NV = 16 * V4 / 64;     // float4s per lane per row block
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        ow[(kg * 4 + r) * OPITCH + dt * 16 + am] = o_acc[rb][dt][r];
    }
    wave_lds_fence();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      int idx = i * 64 + l;
      int row = idx / V4, c4 = idx % V4;
      long qrow = q0 + rb * 16 + row;
      f32x4_t val = *reinterpret_cast<const f32x4_t*>(
          &ow[row * OPITCH + c4 * 4]);
      if (qrow < S)
        *reinterpret_cast<f32x4_t*>(
            &o_part[(row_base + qrow) * D + c4 * 4]) = val;
    }
    wave_lds_fence();  // ow is rewritten by the next row block
  }
}

// One group of D/8 lanes per (bh, q) row; a lane owns 8 consecutive head-dim
// elements: two 16-byte loads per split, one 16-byte bf16 store. The row's
// statistics (at most ATTN_MAX_SPLITS of each) stay in registers. `rows` is
// NBH * S; split s of flat row i sits at (s * rows + i).
template <int D>
__global__ void ATTN_SPLIT_NOPK
__launch_bounds__(256)
attn_fwd_combine_kernel(const float* __restrict__ o_part,
                        const float* __restrict__ m_part,
                        const float* __restrict__ l_part,
                        __hip_bfloat16* __restrict__ O, long rows,
                        int nsplit) {
  constexpr int G = D / 8;
  long row = (long)blockIdx.x * (256 / G) + threadIdx.x / G;
  int c8 = threadIdx.x % G;
  if (row >= rows) return;

  float m[ATTN_MAX_SPLITS];
  float M = -INFINITY;
#pragma unroll
  for (int s = 0; s < ATTN_MAX_SPLITS; ++s) {
    m[s] = s < nsplit ? m_part[s * rows + row] : -INFINITY;
    M = fmaxf(M, m[s]);
  }
  float L = 0.f;
  f32x4_t acc[2];
#pragma unroll
  for (int s = 0; s < ATTN_MAX_SPLITS; ++s) {
    if (s >= nsplit) break;
    float ws = exp2f(m[s] - M);
    float lw = __fmul_rn(l_part[s * rows + row], ws);
    const f32x4_t* src = reinterpret_cast<const f32x4_t*>(
        &o_part[(s * rows + row) * D + c8 * 8]);
    f32x4_t a = src[0], bq = src[1];
    // the first term starts the sums (no 0 + x: that would lose a -0)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pa = __fmul_rn(a[j], ws), pb = __fmul_rn(bq[j], ws);
      acc[0][j] = s == 0 ? pa : __fadd_rn(acc[0][j], pa);
      acc[1][j] = s == 0 ? pb : __fadd_rn(acc[1][j], pb);
    }
    L = s == 0 ? lw : __fadd_rn(L, lw);
  }
  bf16x8_t out;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    __hip_bfloat16 ob = __float2bfloat16(acc[j >> 2][j & 3] / L);
    out[j] = reinterpret_cast<short&>(ob);
  }
  *reinterpret_cast<bf16x8_t*>(
      reinterpret_cast<short*>(O) + row * D + c8 * 8) = out;
}
