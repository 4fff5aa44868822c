// Fused optimizer-apply kernels over flat bucket buffers — the MI355X
// equivalents of TF's ResourceApplyGradientDescent / ResourceApplyKerasMomentum /
// ResourceApplyAdam ops (reference table: autodist/kernel/common/op_info.py:24-68).
//
// One launch updates an ENTIRE gradient bucket (param/grad/state are flat,
// contiguous views — see parallel/buckets.py), so the optimizer step costs
// exactly the read+write HBM traffic of its operands. Kernels are elementwise
// and HBM3E-bound: float4 (16 B/lane) access, 256-thread blocks (4 waves),
// grid-stride loop sized to fill all 8 XCDs.
#include "common.h"
#include <cstdint>

// ------------------------------------------- gradient stream: fp32 or bf16
// The flat SGD / Adam / Adagrad kernels below are templated on the gradient
// element type GT. GT = float is the ordinary bucket path. GT = __hip_bfloat16
// reads the reduce-scattered bf16 WIRE shard of the sharded dense schedule
// directly (parallel/buckets.py): each element is widened to fp32 in
// registers, which is exact (bf16 is the top 16 bits of an fp32), and the
// arithmetic that follows is the same code, so the result is bit-identical to
// cast_back_f32 followed by the fp32 instantiation, without the shard-sized
// fp32 round trip through HBM.
//
// Lane geometry is the same for both: 4 elements per lane per iteration. The
// fp32 streams (param, state) stay at 16 B/lane; the bf16 stream is 8 B/lane
// (one dwordx2, 512 B per wave instruction, still fully coalesced). The
// alternative, 8 elements per lane with a 16 B bf16 load, would double the
// live fp32 registers of every other stream (Adam: p, m, v) for the stream
// that carries only 2 of the kernel's 26 bytes per element, and would give
// the two instantiations different loop bodies; at 4 per lane they share
// one, which is what keeps them bit-identical by construction.
__device__ __forceinline__ void load_grad4(const float* __restrict__ g,
                                           long base, float (&out)[4]) {
  float4 gv = *reinterpret_cast<const float4*>(g + base);
  out[0] = gv.x; out[1] = gv.y; out[2] = gv.z; out[3] = gv.w;
}

__device__ __forceinline__ void load_grad4(
    const __hip_bfloat16* __restrict__ g, long base, float (&out)[4]) {
  uint2 gv = *reinterpret_cast<const uint2*>(g + base);
  out[0] = __uint_as_float(gv.x << 16);
  out[1] = __uint_as_float(gv.x & 0xffff0000u);
  out[2] = __uint_as_float(gv.y << 16);
  out[3] = __uint_as_float(gv.y & 0xffff0000u);
}

__device__ __forceinline__ float load_grad1(const float* __restrict__ g,
                                            long i) {
  return g[i];
}

__device__ __forceinline__ float load_grad1(
    const __hip_bfloat16* __restrict__ g, long i) {
  return __uint_as_float(
      (unsigned)reinterpret_cast<const unsigned short*>(g)[i] << 16);
}

// ---------------------------------------------------------------- SGD
// d = g (+ wd*p); buf = mom*buf + (1-damp)*d (or = d on first step);
// d = nesterov ? d + mom*buf : buf; p -= lr*d
//
// The complements 1-damp, 1-beta, 1-alpha of all kernels in this file are
// formed in double on the host and passed in: 1.f - 0.999f is off by 4.7e-5
// relative (the rounding of 0.999f, magnified 1000x by the subtraction),
// which moved every Adam update by 2.3e-5 relative to torch.optim.
template <bool HAS_MOMENTUM, typename GT>
__global__ void fused_sgd_kernel(float* __restrict__ p,
                                 const GT* __restrict__ g,
                                 float* __restrict__ buf, long n, float lr,
                                 float momentum, float one_minus_damp,
                                 float weight_decay, int nesterov,
                                 int first_step, int maximize) {
  long stride = (long)gridDim.x * blockDim.x * 4;
  for (long base = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; base < n;
       base += stride) {
    if (base + 3 < n) {
      float4 pv = *reinterpret_cast<float4*>(p + base);
      float d[4];
      load_grad4(g, base, d);
      float pr[4] = {pv.x, pv.y, pv.z, pv.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (maximize) d[k] = -d[k];
        d[k] += weight_decay * pr[k];
      }
      if (HAS_MOMENTUM) {
        float4 bv = *reinterpret_cast<float4*>(buf + base);
        float br[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          br[k] = first_step ? d[k] : momentum * br[k] + one_minus_damp * d[k];
          d[k] = nesterov ? d[k] + momentum * br[k] : br[k];
        }
        *reinterpret_cast<float4*>(buf + base) =
            make_float4(br[0], br[1], br[2], br[3]);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) pr[k] -= lr * d[k];
      *reinterpret_cast<float4*>(p + base) =
          make_float4(pr[0], pr[1], pr[2], pr[3]);
    } else {
      for (long i = base; i < n; ++i) {
        float d = load_grad1(g, i);
        if (maximize) d = -d;
        d += weight_decay * p[i];
        if (HAS_MOMENTUM) {
          float b = first_step ? d : momentum * buf[i] + one_minus_damp * d;
          buf[i] = b;
          d = nesterov ? d + momentum * b : b;
        }
        p[i] -= lr * d;
      }
    }
  }
}

// ---------------------------------------------------------------- Adam/AdamW
// adamw: p *= (1 - lr*wd) else g += wd*p
// m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g^2
// p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
template <typename GT>
__global__ void fused_adam_kernel(float* __restrict__ p,
                                  const GT* __restrict__ g,
                                  float* __restrict__ m, float* __restrict__ v,
                                  long n, float lr, float beta1, float beta2,
                                  float one_minus_beta1,
                                  float one_minus_beta2,
                                  float eps, float weight_decay, int adamw,
                                  float bc1, float sqrt_bc2, int maximize) {
  long stride = (long)gridDim.x * blockDim.x * 4;
  float step_size = lr / bc1;
  float wd_mul = 1.f - lr * weight_decay;
  for (long base = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; base < n;
       base += stride) {
    long lim = base + 4 <= n ? 4 : n - base;
    if (lim == 4) {
      float4 pv = *reinterpret_cast<float4*>(p + base);
      float4 mv = *reinterpret_cast<float4*>(m + base);
      float4 vv = *reinterpret_cast<float4*>(v + base);
      float pr[4] = {pv.x, pv.y, pv.z, pv.w};
      float gr[4];
      load_grad4(g, base, gr);
      float mr[4] = {mv.x, mv.y, mv.z, mv.w};
      float vr[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (maximize) gr[k] = -gr[k];
        if (adamw) pr[k] *= wd_mul; else gr[k] += weight_decay * pr[k];
        mr[k] = beta1 * mr[k] + one_minus_beta1 * gr[k];
        vr[k] = beta2 * vr[k] + one_minus_beta2 * gr[k] * gr[k];
        pr[k] -= step_size * mr[k] / (sqrtf(vr[k]) / sqrt_bc2 + eps);
      }
      *reinterpret_cast<float4*>(p + base) = make_float4(pr[0], pr[1], pr[2], pr[3]);
      *reinterpret_cast<float4*>(m + base) = make_float4(mr[0], mr[1], mr[2], mr[3]);
      *reinterpret_cast<float4*>(v + base) = make_float4(vr[0], vr[1], vr[2], vr[3]);
    } else {
      for (long i = base; i < base + lim; ++i) {
        float gr = load_grad1(g, i);
        if (maximize) gr = -gr;
        float pr = p[i];
        if (adamw) pr *= wd_mul; else gr += weight_decay * pr;
        float mr = beta1 * m[i] + one_minus_beta1 * gr;
        float vr = beta2 * v[i] + one_minus_beta2 * gr * gr;
        p[i] = pr - step_size * mr / (sqrtf(vr) / sqrt_bc2 + eps);
        m[i] = mr;
        v[i] = vr;
      }
    }
  }
}

// ------------------------------------------------- compressor cast kernels
// scale+cast fp32 -> bf16 (wire), 8 bf16 out per lane iteration.
__global__ void scale_cast_bf16_kernel(const float* __restrict__ in,
                                       __hip_bfloat16* __restrict__ out,
                                       long n, float scale) {
  long stride = (long)gridDim.x * blockDim.x * 4;
  for (long base = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; base < n;
       base += stride) {
    if (base + 3 < n) {
      float4 v = *reinterpret_cast<const float4*>(in + base);
      __hip_bfloat162 lo = __float22bfloat162_rn({v.x * scale, v.y * scale});
      __hip_bfloat162 hi = __float22bfloat162_rn({v.z * scale, v.w * scale});
      *reinterpret_cast<__hip_bfloat162*>(out + base) = lo;
      *reinterpret_cast<__hip_bfloat162*>(out + base + 2) = hi;
    } else {
      for (long i = base; i < n; ++i) out[i] = __float2bfloat16(in[i] * scale);
    }
  }
}

// cast bf16 wire back to fp32
__global__ void cast_back_f32_kernel(const __hip_bfloat16* __restrict__ in,
                                     float* __restrict__ out, long n) {
  long stride = (long)gridDim.x * blockDim.x * 4;
  for (long base = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; base < n;
       base += stride) {
    if (base + 3 < n) {
      __hip_bfloat162 lo = *reinterpret_cast<const __hip_bfloat162*>(in + base);
      __hip_bfloat162 hi = *reinterpret_cast<const __hip_bfloat162*>(in + base + 2);
      float2 l = __bfloat1622float2(lo);
      float2 h = __bfloat1622float2(hi);
      *reinterpret_cast<float4*>(out + base) = make_float4(l.x, l.y, h.x, h.y);
    } else {
      for (long i = base; i < n; ++i) out[i] = __bfloat162float(in[i]);
    }
  }
}

// fused error-feedback compress: flat += err; wire = bf16(flat*scale);
// err = flat - fp32(wire)/scale   (one pass, reference compressor.py:204-205)
__global__ void ef_compress_kernel(float* __restrict__ flat,
                                   float* __restrict__ err,
                                   __hip_bfloat16* __restrict__ wire, long n,
                                   float scale) {
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    float f = flat[i] + err[i];
    __hip_bfloat16 w = __float2bfloat16(f * scale);
    wire[i] = w;
    err[i] = f - __bfloat162float(w) / scale;
    flat[i] = f;
  }
}

// --------------------------------------------- sparse segment accumulate
// scatter-add rows: out[idx[r]] += vals[r] for row-sparse gradients
// (the SparseConditionalAccumulator dedup-sum, reference
// ps_synchronizer.py:498-535). One thread per (row, col) element.
__global__ void scatter_add_rows_kernel(float* __restrict__ out,
                                        const int64_t* __restrict__ idx,
                                        const float* __restrict__ vals,
                                        long nnz, long dim) {
  long total = nnz * dim;
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    long r = i / dim, c = i % dim;
    atomicAdd(out + idx[r] * dim + c, vals[i]);
  }
}

// rows gather: out[r] = src[idx[r]] (embedding shard gather)
__global__ void gather_rows_kernel(const float* __restrict__ src,
                                   const int64_t* __restrict__ idx,
                                   float* __restrict__ out, long nrows,
                                   long dim) {
  long total = nrows * dim;
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += stride) {
    long r = i / dim, c = i % dim;
    out[i] = src[idx[r] * dim + c];
  }
}

// ---------------------------------------------------------------- Adagrad
// g' = (max? -g : g) + wd*p ; sum += g'^2 ; p -= clr * g'/(sqrt(sum)+eps)
// (clr = lr / (1 + (step-1)*lr_decay), host-computed)
template <typename GT>
__global__ void fused_adagrad_kernel(float* __restrict__ p,
                                     const GT* __restrict__ g,
                                     float* __restrict__ sum, long n,
                                     float clr, float eps,
                                     float weight_decay, int maximize) {
  long stride = (long)gridDim.x * blockDim.x * 4;
  for (long base = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
       base < n; base += stride) {
    if (base + 3 < n) {
      float4 pv = *reinterpret_cast<float4*>(p + base);
      float4 sv = *reinterpret_cast<float4*>(sum + base);
      float pr[4] = {pv.x, pv.y, pv.z, pv.w};
      float gr[4];
      load_grad4(g, base, gr);
      float sr[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float d = maximize ? -gr[k] : gr[k];
        d += weight_decay * pr[k];
        sr[k] += d * d;
        pr[k] -= clr * d / (sqrtf(sr[k]) + eps);
      }
      *reinterpret_cast<float4*>(sum + base) =
          make_float4(sr[0], sr[1], sr[2], sr[3]);
      *reinterpret_cast<float4*>(p + base) =
          make_float4(pr[0], pr[1], pr[2], pr[3]);
    } else {
      for (long i = base; i < n; ++i) {
        float d = load_grad1(g, i);
        if (maximize) d = -d;
        d += weight_decay * p[i];
        sum[i] += d * d;
        p[i] -= clr * d / (sqrtf(sum[i]) + eps);
      }
    }
  }
}

// ---------------------------------------------------------------- RMSprop
// g' = (max? -g : g) + wd*p ; sq = a*sq + (1-a)g'^2 ;
// centered: ga = ga + (1-a)(g'-ga), denom = sqrt(sq - ga^2)+eps
//           else denom = sqrt(sq)+eps
// momentum: buf = mom*buf + g'/denom, p -= lr*buf ; else p -= lr*g'/denom
__global__ void fused_rmsprop_kernel(float* __restrict__ p,
                                     const float* __restrict__ g,
                                     float* __restrict__ sq,
                                     float* __restrict__ ga,   // nullable
                                     float* __restrict__ buf,  // nullable
                                     long n, float lr, float alpha,
                                     float one_minus_alpha,
                                     float eps, float weight_decay,
                                     float momentum, int maximize) {
  long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    float d = maximize ? -g[i] : g[i];
    d += weight_decay * p[i];
    float s = alpha * sq[i] + one_minus_alpha * d * d;
    sq[i] = s;
    float denom;
    if (ga != nullptr) {
      float a = ga[i] + one_minus_alpha * (d - ga[i]);
      ga[i] = a;
      denom = sqrtf(s - a * a) + eps;
    } else {
      denom = sqrtf(s) + eps;
    }
    if (buf != nullptr) {
      float b = momentum * buf[i] + d / denom;
      buf[i] = b;
      p[i] -= lr * b;
    } else {
      p[i] -= lr * d / denom;
    }
  }
}

// ------------------------------------------ row-wise (sparse) optimizer apply
// The SparseApply* table (reference op_info.py:73-117) for UNIQUE rows: for
// each i, r = rows[i] - row_base; rows r of param (and of the state tensors)
// take one optimizer step with gradient row_grads[i]. rows are unique (the
// caller coalesces first), so every (row, column) element has exactly one
// writer and no atomics are needed. An r outside [0, R) is skipped and never
// dereferenced — the shard owner only holds rows [row_base, row_base + R).
// When `out` is given, the updated parameter row is also written to out[i]
// in the same pass (the owner's pull payload; no separate gather).
//
//   SGD:     p -= lr * g
//   Adagrad: s += g^2 ; p -= clr * (g / (sqrt(s) + eps))   (clr host-computed)
//   Adam:    m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g^2 ;
//            p -= lr * (m / bc1 / (sqrt(v)/sqrt(bc2) + eps))
//            (SparseAdam semantics: moments move on touched rows only)
//
// Lane mapping: a power-of-two lane group (1..64 lanes) owns one row and walks
// its D/VEC chunks; a 256-thread block therefore covers 256/group rows, so a
// narrow row (D=8: two float4 chunks) keeps every lane of the wave busy
// instead of leaving 62 of 64 idle. Grid-stride over row groups.
enum { SPARSE_SGD = 0, SPARSE_ADAGRAD = 1, SPARSE_ADAM = 2 };

struct SparseHyper {
  float lr;  // clr for Adagrad
  float beta1, beta2, one_minus_beta1, one_minus_beta2;
  float eps, bc1, sqrt_bc2;
};

template <int OPT>
__device__ __forceinline__ void sparse_update_elem(float& p, float g,
                                                   float& s1, float& s2,
                                                   const SparseHyper& h) {
  if (OPT == SPARSE_SGD) {
    p -= h.lr * g;
  } else if (OPT == SPARSE_ADAGRAD) {
    s1 += g * g;
    p -= h.lr * (g / (sqrtf(s1) + h.eps));
  } else {
    s1 = h.beta1 * s1 + h.one_minus_beta1 * g;
    s2 = h.beta2 * s2 + h.one_minus_beta2 * g * g;
    p -= h.lr * (s1 / h.bc1 / (sqrtf(s2) / h.sqrt_bc2 + h.eps));
  }
}

template <int OPT, int VEC>
__global__ void sparse_apply_rows_kernel(float* __restrict__ p,
                                         const int64_t* __restrict__ rows,
                                         const float* __restrict__ g,
                                         float* __restrict__ s1,   // null: SGD
                                         float* __restrict__ s2,   // Adam only
                                         float* __restrict__ out,  // nullable
                                         long n, long R, long D, long row_base,
                                         int log2_group, SparseHyper h) {
  const int group = 1 << log2_group;
  const int rows_per_block = BLOCK_THREADS >> log2_group;
  const int lane = threadIdx.x & (group - 1);
  const long chunks = D / VEC;
  const long stride = (long)gridDim.x * rows_per_block;
  for (long i = (long)blockIdx.x * rows_per_block + (threadIdx.x >> log2_group);
       i < n; i += stride) {
    const long id = rows[i];
    if (id < row_base || id - row_base >= R) continue;  // not this shard's row
    const long pbase = (id - row_base) * D;
    const long gbase = i * D;
    for (long c = lane; c < chunks; c += group) {
      const long po = pbase + c * VEC;
      const long go = gbase + c * VEC;
      if (VEC == 4) {
        float4 pv = *reinterpret_cast<float4*>(p + po);
        float4 gv = *reinterpret_cast<const float4*>(g + go);
        float4 av = make_float4(0.f, 0.f, 0.f, 0.f), bv = av;
        if (OPT != SPARSE_SGD) av = *reinterpret_cast<float4*>(s1 + po);
        if (OPT == SPARSE_ADAM) bv = *reinterpret_cast<float4*>(s2 + po);
        float pr[4] = {pv.x, pv.y, pv.z, pv.w};
        float gr[4] = {gv.x, gv.y, gv.z, gv.w};
        float ar[4] = {av.x, av.y, av.z, av.w};
        float br[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
          sparse_update_elem<OPT>(pr[k], gr[k], ar[k], br[k], h);
        pv = make_float4(pr[0], pr[1], pr[2], pr[3]);
        *reinterpret_cast<float4*>(p + po) = pv;
        if (OPT != SPARSE_SGD)
          *reinterpret_cast<float4*>(s1 + po) =
              make_float4(ar[0], ar[1], ar[2], ar[3]);
        if (OPT == SPARSE_ADAM)
          *reinterpret_cast<float4*>(s2 + po) =
              make_float4(br[0], br[1], br[2], br[3]);
        if (out != nullptr) *reinterpret_cast<float4*>(out + go) = pv;
      } else {
        float pr = p[po], a = 0.f, b = 0.f;
        if (OPT != SPARSE_SGD) a = s1[po];
        if (OPT == SPARSE_ADAM) b = s2[po];
        sparse_update_elem<OPT>(pr, g[go], a, b, h);
        p[po] = pr;
        if (OPT != SPARSE_SGD) s1[po] = a;
        if (OPT == SPARSE_ADAM) s2[po] = b;
        if (out != nullptr) out[go] = pr;
      }
    }
  }
}
