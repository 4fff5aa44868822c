// Projected-LSTM (LSTMP) cell kernels on gfx950 bf16 matrix cores.
//
// One launch is one time step of one layer. Both kernels are the GEMM
// [B, P] x [P, tile of H] on v_mfma_f32_16x16x32_bf16 (contiguous-8 k-map,
// tests/test_mfma_probe.py) followed by the gate math as the epilogue:
//
//   lstmp_cell_fwd  pre = gx_t + bias + h_prev @ w_hh^T        (4 gates)
//                   i,f,o = sigmoid, g = tanh; c_t = f c_prev + i g;
//                   hc_t = o tanh(c_t)
//   lstmp_cell_bwd  dhc = dh_t @ w_hr[:, tile]; from it, the saved gates,
//                   c_t, c_prev and dc_next: the pre-activation gate
//                   gradients and dc_prev
//
// Work split: a workgroup (256 threads, 4 waves) owns LSTMP_TILE_B = 32 batch
// rows x LSTMP_TILE_H = 32 hidden units; wave w owns the 16 x 16 sub-tile
// (rows 16 (w & 1), units 16 (w >> 1)). In the forward it accumulates ALL
// FOUR gates of its units: w_hh rows j, H + j, 2H + j, 3H + j. In the MFMA
// C layout (col = lane & 15, row = 4 (lane >> 4) + reg) the four gate
// accumulators of one (b, j) are the same lane and register, so the whole
// epilogue runs in registers with no LDS exchange. At B = 128, H = 2048 the
// grid is 4 x 64 = 256 workgroups, one per CU.
//
// Data movement: the A operand (h_prev / dh_t tile, 32 x P) is staged in LDS
// once per workgroup. The B operand streams K = P through LDS in chunks of
// 32, double-buffered: the next chunk's global loads are issued into
// registers before the MFMAs of the current one and stored to the other
// buffer after them; one block barrier per chunk. The forward's B tile is
// 128 w_hh rows (4 gates x 32 units), read along k. The backward reads DOWN
// w_hr's columns (B[k][n] = w_hr[k][j0 + n]); the tile is stored transposed
// so that both kernels read a B fragment as one ds_read_b128. Epilogue
// operands (gx, bias, c_prev / gates, c_t, c_prev, dc_next) are loaded
// before the main loop, so their latency hides behind it.
//
// Ragged tiles (B % 32, H % 32 == 16): loads are clamped to the last valid
// row / unit, stores are masked.
//
// What is NOT here: the projection h_t = hc_t @ w_hr^T reduces over the full
// H, that is across workgroups; fusing it would need a grid-wide barrier
// (or atomics on a bf16 output), which is not wanted on shared machines. It
// stays on hipBLASLt through torch, as do the all-timesteps input projection,
// dh_{t-1} += dgates_t @ w_hh and the four weight / input gradient GEMMs over
// the stacked buffers (ops/fused_lstm.py).
//
// Packed-fp32 VALU forms are switched off for these kernels, for the reason
// given in ce_ops.hip.
#include "common.h"

#define LSTM_NOPK __attribute__((target("no-packed-fp32-ops")))

typedef short lstm_bf16x8 __attribute__((ext_vector_type(8)));
typedef short lstm_bf16x4 __attribute__((ext_vector_type(4)));
typedef float lstm_f32x4 __attribute__((ext_vector_type(4)));

constexpr int LSTMP_TILE_B = 32;   // batch rows per workgroup
constexpr int LSTMP_TILE_H = 32;   // hidden units per workgroup
constexpr int LSTMP_KC = 32;       // k per streamed chunk (one MFMA deep)
constexpr int LSTMP_PAD = 8;       // LDS row padding (shorts)
constexpr int LSTMP_WROW = LSTMP_KC + LSTMP_PAD;
// bytes of the double-buffered B tile: forward (4 gates) and backward
constexpr int LSTMP_W_FWD_BYTES = 2 * 4 * LSTMP_TILE_H * LSTMP_WROW * 2;
constexpr int LSTMP_W_BWD_BYTES = 2 * LSTMP_TILE_H * LSTMP_WROW * 2;
// largest P whose A tile fits next to the forward's B tile in 64 KiB of LDS
constexpr int LSTMP_MAX_P =
    ((65536 - LSTMP_W_FWD_BYTES) / (2 * LSTMP_TILE_B) - LSTMP_PAD) / 32 * 32;

static inline size_t lstmp_lds_bytes(int P, bool fwd) {
  return (size_t)LSTMP_TILE_B * (P + LSTMP_PAD) * 2 +
         (fwd ? LSTMP_W_FWD_BYTES : LSTMP_W_BWD_BYTES);
}

__device__ __forceinline__ LSTM_NOPK float lstm_bf2f(short s) {
  return __builtin_bit_cast(float, ((unsigned)(unsigned short)s) << 16);
}

// round to nearest even; NaN stays NaN
__device__ __forceinline__ LSTM_NOPK short lstm_f2bf(float f) {
  unsigned u = __builtin_bit_cast(unsigned, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (short)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (short)(u >> 16);
}

// 1 / (1 + e^-x): e^-x overflows to +inf for x < -88 and the quotient is 0
__device__ __forceinline__ LSTM_NOPK float lstm_sigmoid(float x) {
  return 1.0f / (1.0f + expf(-x));
}

// overflow-safe tanh: e = e^(-2|x|) lies in (0, 1], so nothing overflows
__device__ __forceinline__ LSTM_NOPK float lstm_tanh(float x) {
  float e = expf(-2.0f * fabsf(x));
  float t = (1.0f - e) / (1.0f + e);
  return copysignf(t, x);
}

// A tile: rows [b0, b0 + 32) of a [B, P] bf16 matrix with row stride lda,
// rows past B clamped to B - 1, into As[32][P + PAD].
__device__ __forceinline__ LSTM_NOPK void lstmp_stage_a(short* As,
                                                        const short* a,
                                                        long lda, int b0,
                                                        int B, int P) {
  const int c8n = P >> 3;
  for (int idx = threadIdx.x; idx < LSTMP_TILE_B * c8n; idx += 256) {
    int r = idx / c8n, c8 = idx - r * c8n;
    int b = min(b0 + r, B - 1);
    *reinterpret_cast<lstm_bf16x8*>(&As[r * (P + LSTMP_PAD) + c8 * 8]) =
        *reinterpret_cast<const lstm_bf16x8*>(&a[(long)b * lda + c8 * 8]);
  }
}

// ------------------------------------------------------------------ forward
__global__ void LSTM_NOPK __launch_bounds__(256)
lstmp_cell_fwd_kernel(const short* __restrict__ gx, long ldgx,
                      const short* __restrict__ h_prev, long ldh,
                      const short* __restrict__ w_hh,
                      const float* __restrict__ bias,
                      const float* __restrict__ c_prev,
                      float* __restrict__ c_out, short* __restrict__ hc_out,
                      short* __restrict__ gates_out, int B, int H, int P) {
  extern __shared__ __attribute__((aligned(16))) short lstm_lds[];
  short* As = lstm_lds;                                   // [32][P + PAD]
  short* Ws = lstm_lds + LSTMP_TILE_B * (P + LSTMP_PAD);  // [2][128][WROW]
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int am = l & 15, kg = l >> 4;
  const int bs = w & 1, us = w >> 1;
  const int b0 = blockIdx.y * LSTMP_TILE_B;
  const int j0 = blockIdx.x * LSTMP_TILE_H;

  // B-tile staging: thread t moves half a row (16 k) of tile row t >> 1;
  // tile row = gate * 32 + unit, units past H clamped to H - 1
  const int srow = t >> 1, scol = (t & 1) * 16;
  const long wrow =
      (long)(srow >> 5) * H + min(j0 + (srow & 31), H - 1);
  const short* wsrc = w_hh + wrow * P + scol;
  short* wdst = Ws + srow * LSTMP_WROW + scol;
  lstm_bf16x8 wreg[2];
#define LSTMP_FWD_LOAD_W(kc)                                                 \
  do {                                                                       \
    wreg[0] = *reinterpret_cast<const lstm_bf16x8*>(wsrc + (kc) * LSTMP_KC); \
    wreg[1] =                                                                \
        *reinterpret_cast<const lstm_bf16x8*>(wsrc + (kc) * LSTMP_KC + 8);   \
  } while (0)
#define LSTMP_FWD_STORE_W(buf)                                               \
  do {                                                                       \
    short* d = wdst + (buf) * 4 * LSTMP_TILE_H * LSTMP_WROW;                 \
    *reinterpret_cast<lstm_bf16x8*>(d) = wreg[0];                            \
    *reinterpret_cast<lstm_bf16x8*>(d + 8) = wreg[1];                        \
  } while (0)
  LSTMP_FWD_LOAD_W(0);

  // epilogue operands of this lane: unit j, batch rows bq + r (both clamped
  // for the loads; the stores below are masked)
  const int j = j0 + us * 16 + am;
  const int jc = min(j, H - 1);
  const int bq = b0 + bs * 16 + kg * 4;
  float pre[4][4], cp[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float bg = bias[g * H + jc];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int b = min(bq + r, B - 1);
      pre[g][r] = lstm_bf2f(gx[(long)b * ldgx + g * H + jc]) + bg;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
    cp[r] = c_prev[(long)min(bq + r, B - 1) * H + jc];

  lstmp_stage_a(As, h_prev, ldh, b0, B, P);
  LSTMP_FWD_STORE_W(0);

  lstm_f32x4 acc[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f},
                       {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const int nk = P / LSTMP_KC;
  const short* arow = As + (bs * 16 + am) * (P + LSTMP_PAD) + kg * 8;
  int cur = 0;
  for (int kc = 0; kc < nk; ++kc) {
    __syncthreads();  // buffer cur (and As) staged; reads of cur ^ 1 done
    const bool has_next = kc + 1 < nk;
    if (has_next) LSTMP_FWD_LOAD_W(kc + 1);
    lstm_bf16x8 af =
        *reinterpret_cast<const lstm_bf16x8*>(arow + kc * LSTMP_KC);
    const short* wb = Ws + (cur * 4 * LSTMP_TILE_H + us * 16 + am) *
                               LSTMP_WROW + kg * 8;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      lstm_bf16x8 bf = *reinterpret_cast<const lstm_bf16x8*>(
          wb + g * LSTMP_TILE_H * LSTMP_WROW);
      acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc[g], 0, 0,
                                                       0);
    }
    if (has_next) LSTMP_FWD_STORE_W(cur ^ 1);
    cur ^= 1;
  }
#undef LSTMP_FWD_LOAD_W
#undef LSTMP_FWD_STORE_W

  if (j >= H) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int b = bq + r;
    if (b >= B) break;
    float ig = lstm_sigmoid(acc[0][r] + pre[0][r]);
    float fg = lstm_sigmoid(acc[1][r] + pre[1][r]);
    float gg = lstm_tanh(acc[2][r] + pre[2][r]);
    float og = lstm_sigmoid(acc[3][r] + pre[3][r]);
    float c = fg * cp[r] + ig * gg;
    c_out[(long)b * H + j] = c;
    hc_out[(long)b * H + j] = lstm_f2bf(og * lstm_tanh(c));
    short* go = gates_out + (long)b * 4 * H + j;
    go[0] = lstm_f2bf(ig);
    go[H] = lstm_f2bf(fg);
    go[2 * H] = lstm_f2bf(gg);
    go[3 * H] = lstm_f2bf(og);
  }
}

// ----------------------------------------------------------------- backward
__global__ void LSTM_NOPK __launch_bounds__(256)
lstmp_cell_bwd_kernel(const short* __restrict__ dh, long lddh,
                      const short* __restrict__ w_hr,
                      const short* __restrict__ gates,
                      const float* __restrict__ c_t,
                      const float* __restrict__ c_prev,
                      const float* __restrict__ dc_next,  // null: zero
                      short* __restrict__ dgates, long lddg,
                      float* __restrict__ dc_prev, int B, int H, int P) {
  extern __shared__ __attribute__((aligned(16))) short lstm_lds[];
  short* As = lstm_lds;                                   // [32][P + PAD]
  short* Ws = lstm_lds + LSTMP_TILE_B * (P + LSTMP_PAD);  // [2][32 n][WROW]
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int am = l & 15, kg = l >> 4;
  const int bs = w & 1, us = w >> 1;
  const int b0 = blockIdx.y * LSTMP_TILE_B;
  const int j0 = blockIdx.x * LSTMP_TILE_H;

  // B-tile staging: thread t moves 4 units of k row t >> 3 and stores them
  // transposed. H % 16 == 0, so a group of 4 units is whole or absent; an
  // absent one re-reads the last valid group.
  const int sk = t >> 3, sn = (t & 7) * 4;
  const short* wsrc = w_hr + (long)sk * H + min(j0 + sn, H - 4);
  short* wdst = Ws + sn * LSTMP_WROW + sk;
  lstm_bf16x4 wreg;
#define LSTMP_BWD_LOAD_W(kc)                          \
  wreg = *reinterpret_cast<const lstm_bf16x4*>(       \
      wsrc + (long)(kc) * LSTMP_KC * H)
#define LSTMP_BWD_STORE_W(buf)                                      \
  do {                                                              \
    short* d = wdst + (buf) * LSTMP_TILE_H * LSTMP_WROW;            \
    _Pragma("unroll") for (int q = 0; q < 4; ++q)                   \
        d[q * LSTMP_WROW] = wreg[q];                                \
  } while (0)
  LSTMP_BWD_LOAD_W(0);

  const int j = j0 + us * 16 + am;
  const int jc = min(j, H - 1);
  const int bq = b0 + bs * 16 + kg * 4;
  float gi[4], gf[4], gg[4], go[4], ct[4], cp[4], dcn[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    long b = min(bq + r, B - 1);
    const short* gp = gates + b * 4 * H + jc;
    gi[r] = lstm_bf2f(gp[0]);
    gf[r] = lstm_bf2f(gp[H]);
    gg[r] = lstm_bf2f(gp[2 * H]);
    go[r] = lstm_bf2f(gp[3 * H]);
    ct[r] = c_t[b * H + jc];
    cp[r] = c_prev[b * H + jc];
    dcn[r] = dc_next ? dc_next[b * H + jc] : 0.f;
  }

  lstmp_stage_a(As, dh, lddh, b0, B, P);
  LSTMP_BWD_STORE_W(0);

  lstm_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int nk = P / LSTMP_KC;
  const short* arow = As + (bs * 16 + am) * (P + LSTMP_PAD) + kg * 8;
  int cur = 0;
  for (int kc = 0; kc < nk; ++kc) {
    __syncthreads();
    const bool has_next = kc + 1 < nk;
    if (has_next) LSTMP_BWD_LOAD_W(kc + 1);
    lstm_bf16x8 af =
        *reinterpret_cast<const lstm_bf16x8*>(arow + kc * LSTMP_KC);
    lstm_bf16x8 bf = *reinterpret_cast<const lstm_bf16x8*>(
        Ws + (cur * LSTMP_TILE_H + us * 16 + am) * LSTMP_WROW + kg * 8);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc, 0, 0, 0);
    if (has_next) LSTMP_BWD_STORE_W(cur ^ 1);
    cur ^= 1;
  }
#undef LSTMP_BWD_LOAD_W
#undef LSTMP_BWD_STORE_W

  if (j >= H) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int b = bq + r;
    if (b >= B) break;
    float dhc = acc[r];
    float tc = lstm_tanh(ct[r]);
    float dc = dhc * go[r] * (1.0f - tc * tc) + dcn[r];
    float d_o = dhc * tc * go[r] * (1.0f - go[r]);
    float d_i = dc * gg[r] * gi[r] * (1.0f - gi[r]);
    float d_f = dc * cp[r] * gf[r] * (1.0f - gf[r]);
    float d_g = dc * gi[r] * (1.0f - gg[r] * gg[r]);
    dc_prev[(long)b * H + j] = dc * gf[r];
    short* dg = dgates + (long)b * lddg + j;
    dg[0] = lstm_f2bf(d_i);
    dg[H] = lstm_f2bf(d_f);
    dg[2 * H] = lstm_f2bf(d_g);
    dg[3 * H] = lstm_f2bf(d_o);
  }
}
