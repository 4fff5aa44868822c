// NeuMF (He et al. 2017: GMF tower + MLP tower + one-logit head, BCE loss) as
// one forward and one backward kernel on the gfx950 fp32 matrix cores.
//
//   H_0    = [mlp_user[u], mlp_item[i]]                       [B, 2E]
//   H_l    = relu(H_{l-1} W_l^T + b_l),  l = 1..L             [B, N_l]
//   z      = w_head . [mf_user[u] * mf_item[i], H_L] + b_head [B]
//   loss   = weight * (max(z, 0) - z y + log1p(exp(-|z|)))    [B]
//
// Everything is fp32: v_mfma_f32_16x16x4_f32 multiplies fp32 exactly and
// accumulates in fp32, so the kernels differ from the torch chain only in the
// order of the sums. Operand layout of that instruction, as psgd_gemm.hip
// uses it: A lane -> (m = lane & 15, k = lane >> 4), B lane -> (k = lane >> 4,
// n = lane & 15), D reg r -> (row = 4 (lane >> 4) + r, col = lane & 15). The
// four k slots of one instruction need not be adjacent columns: a lane
// fetches 16 B (four k of its row) per 16-k chunk and feeds them to four
// consecutive instructions, A and B agreeing on k = k0 + 4 (lane >> 4) + s.
//
// Tiling: a block of 256 threads (4 waves) owns NEUMF_TILE = 32 samples, two
// MFMA row tiles. The activations of the tile live in LDS tiles of
// [32][NEUMF_LD] floats (row pad 4: the 16 rows of an A fetch fall on
// distinct bank groups). A wave owns output column tiles w, w + 4, ... and
// holds both row tiles' accumulators, so each weight fragment fetched from
// global memory / L2 (all blocks read the same <= 160 KB) feeds two MFMAs.
// Widths are multiples of 8: a half-filled 16-column tile and a half 16-k
// chunk are zero-filled in registers.
//
//   neumf_fwd     gather -> LDS, the layers ping-pong between two LDS tiles
//                 with bias + ReLU as the accumulator epilogue, the post-ReLU
//                 H_1..H_L are stored [B, sum N_l] for the backward; the head
//                 is a row dot product by 8 lanes per sample; logits and loss
//                 rows out.
//   neumf_bwd     dz per sample, the GMF row gradients and dH_L from the
//                 head, then per layer (three LDS tiles: G = dH_l masked by
//                 H_l > 0, H_{l-1}, and the next G): db_l (column sums of G),
//                 dW_l = G^T H_{l-1} and dH_{l-1} = G W_l on MFMA. The
//                 per-sample row gradients of the four tables go straight
//                 into [B, D] value buffers, one writer per row. Dense
//                 parameter gradients are per-block partials in a workspace
//                 [blocks, P]: a block walks tiles blockIdx.x, + gridDim.x,
//                 ... and adds into its own slot in that order.
//   neumf_reduce  adds the partials in block order. No atomics anywhere: the
//                 same bits every run.
//
// Packed-fp32 VALU forms are switched off for these kernels, for the reason
// given in ce_ops.hip.
#include "common.h"

#define NCF_NOPK __attribute__((target("no-packed-fp32-ops")))

typedef float ncf_f32x4 __attribute__((ext_vector_type(4)));

constexpr int NEUMF_MAX_LAYERS = 4;
constexpr int NEUMF_MAX_WIDTH = 256;
constexpr int NEUMF_TILE = 32;                   // samples per block
constexpr int NEUMF_LD = NEUMF_MAX_WIDTH + 4;    // LDS row stride (floats)
constexpr int NEUMF_BUF = NEUMF_TILE * NEUMF_LD; // one LDS tile (floats)
constexpr int NEUMF_MAX_BWD_BLOCKS = 256;        // workspace slots at most

// One MLP layer H_l = relu(H_{l-1} W^T + b): W [N, K]. in_off / out_off are
// the columns of H_{l-1} / H_l in the stored activations (in_off unused for
// l = 1, whose input is gathered), w_off / b_off those of dW / db in the flat
// dense gradient.
struct NeumfLayer {
  const float* W;
  const float* b;
  int K, N, in_off, out_off, w_off, b_off;
};

// The layers are named members, not an array: the kernels walk them with
// fixed member accesses so the arguments stay in scalar registers.
struct NeumfArgs {
  const long* users;
  const long* items;
  const float* mf_user;
  const float* mf_item;
  const float* mlp_user;
  const float* mlp_item;
  NeumfLayer l1, l2, l3, l4;
  const float* w_head;               // [mf + N_L]
  const float* b_head;
  const float* labels;               // null: no loss
  const float* weight;               // null: all ones
  long num_users, num_items;
  int B, mf, E, L;
  int act_ld;                        // row stride of the stored activations
  int wl, act_off_last;              // width and column of H_L
  int head_off, P;                   // dw_head in the flat gradient; its size
};

__device__ __forceinline__ NCF_NOPK ncf_f32x4 ncf_mfma(float a, float b,
                                                       ncf_f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// ids of the tile's rows into LDS; rows past B repeat row B - 1 (nothing is
// stored for them). Ids within the tables are the caller's contract; they are
// clamped so that a bad one cannot read outside the table.
__device__ __forceinline__ NCF_NOPK void ncf_load_ids(const NeumfArgs& a,
                                                      int row0, long* uid,
                                                      long* iid) {
  const int t = threadIdx.x;
  if (t < 2 * NEUMF_TILE) {
    const int r = t & (NEUMF_TILE - 1);
    const int rc = min(row0 + r, a.B - 1);
    if (t < NEUMF_TILE)
      uid[r] = min(max(a.users[rc], 0L), a.num_users - 1);
    else
      iid[r] = min(max(a.items[rc], 0L), a.num_items - 1);
  }
}

// X[r][0 .. 2E) = [mlp_user[u_r], mlp_item[i_r]], 16 B per lane
__device__ __forceinline__ NCF_NOPK void ncf_gather(const NeumfArgs& a,
                                                    const long* uid,
                                                    const long* iid,
                                                    float* X) {
  const int v = a.E >> 2;
  for (int idx = threadIdx.x; idx < NEUMF_TILE * 2 * v; idx += 256) {
    const int r = idx / (2 * v), c = idx - r * 2 * v;
    const float* src = c < v ? a.mlp_user + uid[r] * a.E + 4 * c
                             : a.mlp_item + iid[r] * a.E + 4 * (c - v);
    *reinterpret_cast<float4*>(X + r * NEUMF_LD + 4 * c) =
        *reinterpret_cast<const float4*>(src);
  }
}

// X[r][0 .. n) = H_l rows of the tile from the stored activations
__device__ __forceinline__ NCF_NOPK void ncf_load_act(
    const NeumfArgs& a, const float* __restrict__ acts, int row0, int width,
    int off, float* X) {
  const int v = width >> 2;
  for (int idx = threadIdx.x; idx < NEUMF_TILE * v; idx += 256) {
    const int r = idx / v, c = idx - r * v;
    const long row = min(row0 + r, a.B - 1);
    *reinterpret_cast<float4*>(X + r * NEUMF_LD + 4 * c) =
        *reinterpret_cast<const float4*>(acts + row * a.act_ld + off +
                                         4 * c);
  }
}

// out[32, N] = X[32, K] W[N, K]^T. epi(row tile, column tile, accumulator).
template <typename Epi>
__device__ __forceinline__ NCF_NOPK void ncf_gemm_nt(
    const float* X, const float* __restrict__ W, int K, int N, Epi epi) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int am = l & 15, kg = l >> 4;
  const float4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int ct = w; ct * 16 < N; ct += 4) {
    const int n = ct * 16 + am;
    const bool nok = n < N;
    const float* wrow = W + (long)min(n, N - 1) * K + 4 * kg;
    const float* x0 = X + am * NEUMF_LD + 4 * kg;
    const float* x1 = x0 + 16 * NEUMF_LD;
    ncf_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    // the next chunk's weights are in flight during this chunk's MFMAs
    float4 bv = zero;
    if (nok && 4 * kg < K) bv = *reinterpret_cast<const float4*>(wrow);
    for (int k0 = 0; k0 < K; k0 += 16) {
      const bool kok = k0 + 4 * kg < K;
      float4 bn = zero, a0 = zero, a1 = zero;
      if (nok && k0 + 16 + 4 * kg < K)
        bn = *reinterpret_cast<const float4*>(wrow + k0 + 16);
      if (kok) {
        a0 = *reinterpret_cast<const float4*>(x0 + k0);
        a1 = *reinterpret_cast<const float4*>(x1 + k0);
      }
      acc0 = ncf_mfma(a0.x, bv.x, acc0);
      acc1 = ncf_mfma(a1.x, bv.x, acc1);
      acc0 = ncf_mfma(a0.y, bv.y, acc0);
      acc1 = ncf_mfma(a1.y, bv.y, acc1);
      acc0 = ncf_mfma(a0.z, bv.z, acc0);
      acc1 = ncf_mfma(a1.z, bv.z, acc1);
      acc0 = ncf_mfma(a0.w, bv.w, acc0);
      acc1 = ncf_mfma(a1.w, bv.w, acc1);
      bv = bn;
    }
    epi(0, ct, acc0);
    epi(1, ct, acc1);
  }
}

// out[32, K] = G[32, N] W[N, K]: the B lane (k = n0 + 4 kg + s, column kc)
// reads W[k][kc], 64 B per row of W across the 16 lanes of a group.
template <typename Epi>
__device__ __forceinline__ NCF_NOPK void ncf_gemm_nn(
    const float* G, const float* __restrict__ W, int N, int K, Epi epi) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int am = l & 15, kg = l >> 4;
  const float4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int ct = w; ct * 16 < K; ct += 4) {
    const int kc = ct * 16 + am;
    const bool cok = kc < K;
    const float* wcol = W + min(kc, K - 1) + (long)(4 * kg) * K;
    const float* g0 = G + am * NEUMF_LD + 4 * kg;
    const float* g1 = g0 + 16 * NEUMF_LD;
    ncf_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    auto load_b = [&](int n0) {
      float4 v = zero;
      if (cok && n0 + 4 * kg < N) {
        const float* p = wcol + (long)n0 * K;
        v.x = p[0];
        v.y = p[K];
        v.z = p[2 * (long)K];
        v.w = p[3 * (long)K];
      }
      return v;
    };
    float4 bv = load_b(0);
    for (int n0 = 0; n0 < N; n0 += 16) {
      const bool nok = n0 + 4 * kg < N;
      const float4 bn = load_b(n0 + 16);
      float4 a0 = zero, a1 = zero;
      if (nok) {
        a0 = *reinterpret_cast<const float4*>(g0 + n0);
        a1 = *reinterpret_cast<const float4*>(g1 + n0);
      }
      acc0 = ncf_mfma(a0.x, bv.x, acc0);
      acc1 = ncf_mfma(a1.x, bv.x, acc1);
      acc0 = ncf_mfma(a0.y, bv.y, acc0);
      acc1 = ncf_mfma(a1.y, bv.y, acc1);
      acc0 = ncf_mfma(a0.z, bv.z, acc0);
      acc1 = ncf_mfma(a1.z, bv.z, acc1);
      acc0 = ncf_mfma(a0.w, bv.w, acc0);
      acc1 = ncf_mfma(a1.w, bv.w, acc1);
      bv = bn;
    }
    epi(0, ct, acc0);
    epi(1, ct, acc1);
  }
}

// out[N, K] (+)= G[32, N]^T Hp[32, K], the reduction over the tile's 32
// samples in 8 MFMA steps. A wave owns row tiles nt = w, w + 4, ... of the
// output and keeps their A fragments for the walk over the column tiles.
__device__ __forceinline__ NCF_NOPK void ncf_gemm_tn(const float* G,
                                                     const float* Hp, int N,
                                                     int K,
                                                     float* __restrict__ out,
                                                     bool first) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int am = l & 15, kg = l >> 4;
  for (int nt = w; nt * 16 < N; nt += 4) {
    const int n = nt * 16 + am;
    float af[8];
#pragma unroll
    for (int s = 0; s < 8; ++s)
      af[s] = n < N ? G[(4 * s + kg) * NEUMF_LD + n] : 0.f;
    for (int kt = 0; kt * 16 < K; ++kt) {
      const int kc = kt * 16 + am;
      const bool cok = kc < K;
      ncf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const float bv = cok ? Hp[(4 * s + kg) * NEUMF_LD + kc] : 0.f;
        acc = ncf_mfma(af[s], bv, acc);
      }
      if (cok) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int nr = nt * 16 + 4 * kg + r;
          if (nr < N) {
            float* p = out + (long)nr * K + kc;
            *p = first ? acc[r] : *p + acc[r];
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------ forward
__global__ void NCF_NOPK __launch_bounds__(256)
neumf_fwd_kernel(NeumfArgs a, float* __restrict__ logits,
                 float* __restrict__ loss_rows, float* __restrict__ acts) {
  __shared__ __attribute__((aligned(16))) float S[2 * NEUMF_BUF];
  __shared__ long uid[NEUMF_TILE], iid[NEUMF_TILE];
  const int t = threadIdx.x, kg = (t & 63) >> 4, am = t & 15;
  const int row0 = blockIdx.x * NEUMF_TILE;
  ncf_load_ids(a, row0, uid, iid);
  __syncthreads();
  ncf_gather(a, uid, iid, S);
  __syncthreads();
  int cur = 0;
  auto layer = [&](const NeumfLayer& ly) __attribute__((always_inline)) {
    const int N = ly.N;
    const float* X = S + cur * NEUMF_BUF;
    float* Y = S + (cur ^ 1) * NEUMF_BUF;
    const float* bias = ly.b;
    const int aoff = ly.out_off;
    ncf_gemm_nt(X, ly.W, ly.K, N, [&](int rt, int ct, ncf_f32x4 acc) {
      const int col = ct * 16 + am;
      if (col < N) {
        const float bc = bias[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = rt * 16 + 4 * kg + r;
          const float v = fmaxf(acc[r] + bc, 0.f);
          Y[row * NEUMF_LD + col] = v;
          if (acts && row0 + row < a.B)
            acts[(long)(row0 + row) * a.act_ld + aoff + col] = v;
        }
      }
    });
    __syncthreads();
    cur ^= 1;
  };
  layer(a.l1);
  if (a.L >= 2) layer(a.l2);
  if (a.L >= 3) layer(a.l3);
  if (a.L >= 4) layer(a.l4);
  // head: 8 lanes per sample, partial dots added in a fixed xor order
  const float* X = S + cur * NEUMF_BUF;
  const int r = t >> 3, q = t & 7, wl = a.wl;
  const float* pu = a.mf_user + uid[r] * a.mf;
  const float* pi = a.mf_item + iid[r] * a.mf;
  float s = 0.f;
  for (int j = q; j < a.mf; j += 8) s += a.w_head[j] * (pu[j] * pi[j]);
  for (int k = q; k < wl; k += 8)
    s += a.w_head[a.mf + k] * X[r * NEUMF_LD + k];
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 4, 64);
  const int row = row0 + r;
  if (q == 0 && row < a.B) {
    const float z = s + a.b_head[0];
    logits[row] = z;
    if (a.labels) {
      float v = (fmaxf(z, 0.f) - z * a.labels[row]) + log1pf(expf(-fabsf(z)));
      if (a.weight) v *= a.weight[row];
      loss_rows[row] = v;
    }
  }
}

// ----------------------------------------------------------------- backward
// Layer l's descriptor, read from the kernel argument segment (the NeumfArgs
// is the kernel's first argument, at offset 0) when its turn comes: holding
// all four in scalar registers across the tile loop spills them.
__device__ __forceinline__ NCF_NOPK NeumfLayer
ncf_kernarg_layer(const NeumfArgs& a, int l) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const __attribute__((address_space(4))) char* karg_bytes;
  typedef const __attribute__((address_space(4))) NeumfLayer* karg_layer;
  const karg_layer p =
      (karg_layer)((karg_bytes)__builtin_amdgcn_kernarg_segment_ptr() +
                   offsetof(NeumfArgs, l1)) + (l - 1);
  NeumfLayer ly;
  ly.W = p->W;
  ly.b = p->b;
  ly.K = p->K;
  ly.N = p->N;
  ly.in_off = p->in_off;
  ly.out_off = p->out_off;
  ly.w_off = p->w_off;
  ly.b_off = p->b_off;
  return ly;
#else
  return (&a.l1)[l - 1];
#endif
}

// ws slot of this block: [P] floats; `first` writes, later tiles add.
__device__ __forceinline__ NCF_NOPK void ncf_acc(float* p, float v,
                                                 bool first) {
  *p = first ? v : *p + v;
}

__global__ void NCF_NOPK __launch_bounds__(256)
neumf_bwd_kernel(NeumfArgs a, const float* __restrict__ logits,
                 const float* __restrict__ acts,
                 const float* __restrict__ g_logits,
                 const float* __restrict__ g_loss, float* __restrict__ d_mfu,
                 float* __restrict__ d_mfi, float* __restrict__ d_mlpu,
                 float* __restrict__ d_mlpi, float* __restrict__ ws,
                 int ntiles) {
  __shared__ __attribute__((aligned(16))) float S[3 * NEUMF_BUF];
  __shared__ long uid[NEUMF_TILE], iid[NEUMF_TILE];
  __shared__ float dz[NEUMF_TILE];
  const int t = threadIdx.x, kg = (t & 63) >> 4, am = t & 15;
  float* slot = ws + (long)blockIdx.x * a.P;
  const int wl = a.wl;
  bool first = true;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int row0 = tile * NEUMF_TILE;
    ncf_load_ids(a, row0, uid, iid);
    if (t < NEUMF_TILE) {
      const int row = row0 + t;
      float d = 0.f;
      if (row < a.B) {
        if (g_logits) d = g_logits[row];
        if (g_loss && a.labels) {
          const float z = logits[row];
          const float e = expf(-fabsf(z));
          const float sg = (z >= 0.f ? 1.f : e) / (1.f + e);
          float gl = g_loss[row];
          if (a.weight) gl *= a.weight[row];
          d += gl * (sg - a.labels[row]);
        }
      }
      dz[t] = d;
    }
    int g = 1, hp = 0, gn = 2;  // LDS tiles: G, H_{l-1}, next G
    ncf_load_act(a, acts, row0, wl, a.act_off_last, S + hp * NEUMF_BUF);
    __syncthreads();

    // head: G_L = dz w_head[mf + k] [H_L > 0]; dw_head, db_head partials
    for (int k = t; k < wl; k += 256) {
      const float wk = a.w_head[a.mf + k];
      const float* h = S + hp * NEUMF_BUF + k;
      float* go = S + g * NEUMF_BUF + k;
      float s = 0.f;
#pragma unroll 8
      for (int r = 0; r < NEUMF_TILE; ++r) {
        const float hv = h[r * NEUMF_LD];
        s += dz[r] * hv;
        go[r * NEUMF_LD] = hv > 0.f ? dz[r] * wk : 0.f;
      }
      ncf_acc(slot + a.head_off + a.mf + k, s, first);
    }
    for (int j = t; j < a.mf; j += 256) {
      const float wj = a.w_head[j];
      float s = 0.f;
#pragma unroll 8
      for (int r = 0; r < NEUMF_TILE; ++r) {
        const float pu = a.mf_user[uid[r] * a.mf + j];
        const float pi = a.mf_item[iid[r] * a.mf + j];
        const float d = dz[r] * wj;
        s += dz[r] * (pu * pi);
        if (row0 + r < a.B) {
          d_mfu[(long)(row0 + r) * a.mf + j] = d * pi;
          d_mfi[(long)(row0 + r) * a.mf + j] = d * pu;
        }
      }
      ncf_acc(slot + a.head_off + j, s, first);
    }
    if (t == 0) {
      float s = 0.f;
      for (int r = 0; r < NEUMF_TILE; ++r) s += dz[r];
      ncf_acc(slot + a.head_off + a.mf + wl, s, first);
    }

    auto layer = [&](const NeumfLayer& ly, bool last)
                     __attribute__((always_inline)) {
      const int K = ly.K, N = ly.N;
      __syncthreads();  // G written; the tile that becomes H_{l-1} is free
      float* Hp = S + hp * NEUMF_BUF;
      if (!last)
        ncf_load_act(a, acts, row0, K, ly.in_off, Hp);
      else
        ncf_gather(a, uid, iid, Hp);
      __syncthreads();
      const float* G = S + g * NEUMF_BUF;
      for (int n = t; n < N; n += 256) {
        float s = 0.f;
#pragma unroll 8
        for (int r = 0; r < NEUMF_TILE; ++r) s += G[r * NEUMF_LD + n];
        ncf_acc(slot + ly.b_off + n, s, first);
      }
      ncf_gemm_tn(G, Hp, N, K, slot + ly.w_off, first);
      float* Gn = S + gn * NEUMF_BUF;
      ncf_gemm_nn(G, ly.W, N, K, [&](int rt, int ct, ncf_f32x4 acc) {
        const int col = ct * 16 + am;
        if (col < K) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = rt * 16 + 4 * kg + r;
            if (!last) {
              Gn[row * NEUMF_LD + col] =
                  Hp[row * NEUMF_LD + col] > 0.f ? acc[r] : 0.f;
            } else if (row0 + row < a.B) {
              if (col < a.E)
                d_mlpu[(long)(row0 + row) * a.E + col] = acc[r];
              else
                d_mlpi[(long)(row0 + row) * a.E + col - a.E] = acc[r];
            }
          }
        }
      });
      const int old_g = g;
      g = gn;
      gn = hp;
      hp = old_g;
    };
    for (int l = a.L; l >= 1; --l) {
      const NeumfLayer ly = ncf_kernarg_layer(a, l);
      layer(ly, l == 1);
    }
    __syncthreads();  // the next tile overwrites ids, dz and the LDS tiles
    first = false;
  }
}

// dense[p] = sum of the blocks' partials, in block order
__global__ void NCF_NOPK __launch_bounds__(256)
neumf_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dense,
                    int P, int nblk) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  float s = 0.f;
#pragma unroll 8
  for (int b = 0; b < nblk; ++b) s += ws[(long)b * P + p];
  dense[p] = s;
}
