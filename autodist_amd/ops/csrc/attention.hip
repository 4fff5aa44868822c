// Fused attention FORWARD on gfx950 matrix cores.
//
// O = dropout(softmax(Q K^T / sqrt(D) + mask)) V for [B, H, S, D] bf16,
// D = 64, S % 32 == 0. mask is an optional ADDITIVE key-padding mask
// [B, 1, 1, S] (the BERT attention_mask form); dropout uses a counter-based
// hash of (seed, bh, q, k) so the backward regenerates the identical mask
// without materializing S x S state (flash-attention-style).
//
// v3 structure (4 waves x 16-query rows = 64-query tile per block):
//   * 64-KEY K/V tiles staged in DOUBLE-BUFFERED LDS, consumed by all 4
//     waves: one block barrier per 64 keys (the v2 design paid 3 barriers
//     per 32 keys and was barrier-bound at S >= 512). Next tile's global
//     loads are issued into the other buffer before computing the current
//     one, so HBM latency overlaps the MFMA work.
//   * V is staged TRANSPOSED so P@V B-fragments are single ds_read_b128s;
//     P is staged bf16 per wave (C-layout write, A-layout read) with a
//     wave-local s_waitcnt fence instead of a block barrier.
//   * QK^T and P@V on v_mfma_f32_16x16x32_bf16 (contiguous-8 k-map; see
//     tests/test_mfma_probe.py for the measured layout contract).
//   * online softmax in fp32: per-row running max m / sum l, row
//     reductions via shfl_xor over the 16-lane C-column group. l
//     accumulates the UNdropped probabilities (torch semantics: dropout
//     after softmax); the 1/(1-p) rescale is folded into the epilogue.
#include "common.h"

typedef short bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

#define ATTN_D 64
#define KPAD 8  // LDS row padding (shorts) to stagger banks


// order LDS writes before reads WITHIN one wave (cheaper than a block
// barrier; wavefront lockstep makes it safe once the counters drain)
__device__ __forceinline__ void wave_lds_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// dropout: drop_hash (common.h), a pure function of (seed, bh, q, k), so
// forward and both backward kernels regenerate the identical mask.

// 256 threads (4 waves); each wave owns RB x 16 query rows, so a block
// covers 64*RB queries. K/V tiles are shared by all 4 waves from LDS, so
// doubling RB HALVES the K/V re-read traffic per query — the kernel is
// K/V-bandwidth-bound at S >= 512 (measured: SQ busy 4.5%, ~2 TB/s of
// tile re-reads; SDPA's advantage was exactly its larger q-tile).
// The grid is launched 1-D as qb * (B*H) + bh: consecutive workgroup ids
// round-robin across the 8 XCDs, so all q-blocks of one (b,h) — which
// re-read the SAME K/V — land on the SAME XCD's L2 when B*H % 8 == 0
// (XCD-aware swizzle; B*H is the fast dimension mod 8).
template <int RB, int D>
__global__ void
__launch_bounds__(256, D == 64 ? 2 : 1)
attn_fwd_kernel(const __hip_bfloat16* __restrict__ Q,
                const __hip_bfloat16* __restrict__ K,
                const __hip_bfloat16* __restrict__ V,
                __hip_bfloat16* __restrict__ O,
                const float* __restrict__ mask, long S, long H, long NBH,
                long q_sb, long q_sh, long q_ss,  // element strides: Q/K/V
                long k_sb, long k_sh, long k_ss,  // may be VIEWS of the
                long v_sb, long v_sh, long v_ss,  // fused qkv projection
                float scale, float p_drop, unsigned int seed) {
  __shared__ short Ks[2][64][D + KPAD];
  __shared__ short VsT[2][D][64 + KPAD];  // transposed: B-frag reads are
                                          // one ds_read_b128
  __shared__ short Pw[4][16][64 + KPAD];  // per-wave bf16 P staging
  int t = threadIdx.x;
  int w = t >> 6;        // wave 0..3
  int l = t & 63;        // lane
  long bh = (long)blockIdx.x % NBH;            // XCD swizzle (see above)
  long qb = (long)blockIdx.x / NBH;
  long q0 = qb * (64 * RB) + w * (16 * RB);    // this wave's RB*16 q rows
  long b = bh / H, hh = bh % H;
  const short* q_p = reinterpret_cast<const short*>(Q) + b * q_sb + hh * q_sh;
  const short* k_p = reinterpret_cast<const short*>(K) + b * k_sb + hh * k_sh;
  const short* v_p = reinterpret_cast<const short*>(V) + b * v_sb + hh * v_sh;
  short* o_p = reinterpret_cast<short*>(O) + bh * S * D;
  const float* m_p = mask ? mask + (bh / H) * S : nullptr;

  constexpr int NC = D / 32;   // A/B k-chunks along the head dim
  constexpr int ND = D / 16;   // C d-tiles
  int am = l & 15;       // A-fragment m index / C column index
  int kg = l >> 4;       // k-group (0..3)
  const unsigned int thresh =
      (unsigned int)fminf(p_drop * 4294967296.0f, 4294967040.0f);
  const bool do_drop = p_drop > 0.0f;
  const float scale2 = scale * ATTN_LOG2E;  // exp2-domain logit scale

  // Q fragments: q row (q0+rb*16+am) clamped for partial tiles
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
  f32x4_t o_acc[RB][ND];  // d-tiles of 16 cols each
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

  // cooperative 64xD K/V stage: 256 threads x one row-quarter (D/4 shorts
  // = D/32 bf16x8 loads) each -> thread t stages row (t>>2)
  int srow = t >> 2, scol = (t & 3) * (D / 4);
  constexpr int NH = D / 32;  // bf16x8 chunks per thread

  bf16x8_t kreg[NH], vreg[NH];
  auto load_tile = [&](long kt) {  // issue global loads into registers
    int krow = kt + srow < S ? (int)kt + srow : (int)S - 1;
#pragma unroll
    for (int half = 0; half < NH; ++half) {
      kreg[half] = *reinterpret_cast<const bf16x8_t*>(
          &k_p[krow * k_ss + scol + half * 8]);
      vreg[half] = *reinterpret_cast<const bf16x8_t*>(
          &v_p[krow * v_ss + scol + half * 8]);
    }
  };
  auto store_tile = [&](int buf) {  // registers -> LDS (after compute)
#pragma unroll
    for (int half = 0; half < NH; ++half) {
      *reinterpret_cast<bf16x8_t*>(&Ks[buf][srow][scol + half * 8]) =
          kreg[half];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        VsT[buf][scol + half * 8 + j][srow] = vreg[half][j];
    }
  };

  load_tile(0);
  store_tile(0);
  int cur = 0;
  for (long kt = 0; kt < S; kt += 64) {
    __syncthreads();  // current buffer staged; previous reads done
    bool has_next = kt + 64 < S;
    if (has_next) load_tile(kt + 64);  // overlap HBM with the MFMAs below

    float mv2[4], oob[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      int key = (int)kt + h * 16 + am;
      mv2[h] = (m_p && key < (int)S) ? m_p[key] * ATTN_LOG2E : 0.f;
      oob[h] = key < (int)S ? 0.f : -1e30f;  // partial last tile
    }

#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      // ---- S tile = Q[16] x K[64]^T : four 16x16 C tiles (key quarters)
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
      // online softmax in the exp2 domain (v_exp_f32 IS exp2)
      float sv[4][4];  // [h][r]
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
        if (do_drop) {
          unsigned int qrow = (unsigned int)(q0 + rb * 16 + kg * 4 + r);
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            if (drop_hash(seed, (unsigned int)bh, qrow,
                          (unsigned int)(kt + h * 16 + am)) < thresh)
              sv[h][r] = 0.f;
          }
        }
      }
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o_acc[rb][dt][r] *= alpha[r];
      }
      // ---- stage (dropped) P bf16 through per-wave LDS: C-write, A-read
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
      // ---- O += P @ V : per 16-col d tile, two k-chunks of 32 keys
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
      wave_lds_fence();  // Pw reused by the next row block / iteration
    }
    if (has_next) store_tile(1 - cur);
    cur = 1 - cur;
  }
  // ---- epilogue: normalize (+ dropout keep-rescale) + store
  float rkeep = do_drop ? 1.0f / (1.0f - p_drop) : 1.0f;
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        long qrow = q0 + rb * 16 + kg * 4 + r;
        if (qrow >= S) continue;
        float val = o_acc[rb][dt][r] / l_run[rb][r] * rkeep;
        __hip_bfloat16 ob = __float2bfloat16(val);
        o_p[qrow * D + dt * 16 + am] = reinterpret_cast<short&>(ob);
      }
    }
  }
}

// debug/testing: materialize the dropout keep-mask (1=kept) the kernels
// derive from (seed, bh, q, k) — lets tests build an exact torch reference.
__global__ void attn_dropmask_kernel(unsigned char* __restrict__ out, long S,
                                     float p_drop, unsigned int seed) {
  long bh = blockIdx.y;
  long q = blockIdx.x;
  unsigned int thresh =
      (unsigned int)fminf(p_drop * 4294967296.0f, 4294967040.0f);
  for (long k = threadIdx.x; k < S; k += blockDim.x) {
    out[(bh * S + q) * S + k] =
        drop_hash(seed, (unsigned int)bh, (unsigned int)q,
                  (unsigned int)k) >= thresh;
  }
}
