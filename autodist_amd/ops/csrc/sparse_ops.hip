// Sort-free, bit-reproducible coalesce of row-sparse gradients.
//
//   in : ids[n] int64 in [0, R), vals[n, D] fp32, scale
//   out: uniq[n] int64   ascending unique ids in [0, m), then -1
//        out[n, D] fp32  row s < m = sum of the rows of id uniq[s], rest 0
//        count[1] int32  m
//
// Summation rule: out[slot(id)] = sum of round_fp32(vals[i] * scale) over
// the inputs i with ids[i] == id, added in ASCENDING i, one fp32 add at a
// time, starting from the first addend. The multiply is never contracted into
// the add. That is what a sequential CPU loop computes, so the result is one
// fixed set of bits. No float atomics anywhere; the integer atomics below
// (bitmap bits, counters, cursors) only decide where intermediate integers
// land, never what the output holds.
//
// The table height R is known, so the dedup needs no sort: a bitmap over row
// ids gives the sorted unique ids and, by popcount ranking, every id's output
// slot. Launch chain (all on the caller's stream):
//
//   coalesce_mark    one thread per input: atomicOr of the id's bit; clears
//                    the per-call slot counters and the segment cursor.
//   coalesce_totals  popcount total of each 256-word bitmap block.
//   coalesce_scan    one block: exclusive scan of the block totals in place
//                    (chunks of 256 with a running carry), writes count.
//   coalesce_emit    per 256-word block: exclusive scan of the word
//                    popcounts + block base -> prefix[w]; the thread that owns
//                    word w writes 32w + bit for each set bit to
//                    uniq[prefix[w] + k]: sorted by construction, one writer
//                    per element.
//   coalesce_count   slot(i) = prefix[w] + popc(bitmap[w] & ((1 << b) - 1)),
//                    kept in slot[i]; integer atomicAdd of cnt[slot].
//   coalesce_alloc   one thread per slot: claims cnt[s] entries of perm by an
//                    integer bump cursor (segment order is arbitrary and
//                    irrelevant).
//   coalesce_place   input i is put into its slot's segment by an integer
//                    atomic cursor (order inside a segment is arbitrary at
//                    this point); each input stores 0 to its bitmap word, so
//                    the workspace is all-zero again for the next call.
//                    (coalesce_count is the last READER of the bitmap, but a
//                    thread there cannot clear a word other threads of the
//                    same launch still have to read; the clear therefore sits
//                    one launch later.)
//   coalesce_sum     a power-of-two lane group per output slot (sized from D
//                    as sparse_apply_rows_kernel does) adds the slot's rows in
//                    ascending input position:
//                      c*c <= n/G: every lane selects the next-larger
//                                position of the slot's segment by a min-scan
//                                over its c entries (group-uniform loads; c
//                                is 1 or 2 for almost every slot);
//                      else    : the group walks slot[0..n) in order, a
//                                ballot per G inputs yields the contributors
//                                of this slot, lowest bit first. A heavy slot
//                                costs n/G loads per lane (8 in flight)
//                                instead of c*c.
//                    Pad rows [m, n) are zero-filled and uniq[m..n) set to -1
//                    here, not by a fill launch.
//
// An id outside [0, R) is the caller's contract violation; the kernels skip
// it without a dereference (slot -1), as sparse_apply_rows_kernel does.
//
// Workspace (int32, cached per table height by the caller, all-zero bitmap
// between calls): bitmap[W] | prefix[W] | blocksum[ceil(W/256)], W =
// ceil(R/32). Per-call scratch (int32): slot[n] | cnt[n] | start[n] |
// perm[n] | cursor.
//
// Packed-fp32 VALU forms are switched off for these kernels, for the reason
// given in ce_ops.hip.
#include "common.h"
#include <cstdint>

#define SPO_NOPK __attribute__((target("no-packed-fp32-ops")))

constexpr int SPO_WALK_U = 8;  // slot[] loads in flight per lane in the walk

// Exclusive scan of one int per thread over a 256-thread block (Hillis-Steele
// in LDS). Returns the exclusive prefix; total = sum over the block. lds is
// free for reuse on return.
__device__ __forceinline__ SPO_NOPK int spo_block_scan(int v, int* lds,
                                                       int& total) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
#pragma unroll
  for (int off = 1; off < BLOCK_THREADS; off <<= 1) {
    int a = t >= off ? lds[t - off] : 0;
    __syncthreads();
    lds[t] += a;
    __syncthreads();
  }
  int incl = lds[t];
  total = lds[BLOCK_THREADS - 1];
  __syncthreads();
  return incl - v;
}

__global__ void __launch_bounds__(BLOCK_THREADS) SPO_NOPK
coalesce_mark_kernel(const int64_t* __restrict__ ids,
                     unsigned int* __restrict__ bitmap,
                     int* __restrict__ cnt, int* __restrict__ cursor, long n,
                     long R) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    cnt[i] = 0;
    if (i == 0) *cursor = 0;
    const long id = ids[i];
    if (id < 0 || id >= R) continue;
    atomicOr(bitmap + (id >> 5), 1u << (id & 31));
  }
}

__global__ void __launch_bounds__(BLOCK_THREADS) SPO_NOPK
coalesce_totals_kernel(const unsigned int* __restrict__ bitmap,
                       int* __restrict__ blocksum, long W) {
  __shared__ int lds[BLOCK_THREADS / WAVE_SIZE];
  const long nblk = (W + BLOCK_THREADS - 1) / BLOCK_THREADS;
  for (long b = blockIdx.x; b < nblk; b += gridDim.x) {
    const long w = b * BLOCK_THREADS + threadIdx.x;
    int v = w < W ? __popc(bitmap[w]) : 0;
#pragma unroll
    for (int off = WAVE_SIZE / 2; off > 0; off >>= 1)
      v += __shfl_xor(v, off, WAVE_SIZE);
    if ((threadIdx.x & (WAVE_SIZE - 1)) == 0)
      lds[threadIdx.x / WAVE_SIZE] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      int s = 0;
#pragma unroll
      for (int k = 0; k < BLOCK_THREADS / WAVE_SIZE; ++k) s += lds[k];
      blocksum[b] = s;
    }
    __syncthreads();
  }
}

// One block. blocksum[nblk] becomes its exclusive scan; count = grand total.
__global__ void __launch_bounds__(BLOCK_THREADS) SPO_NOPK
coalesce_scan_kernel(int* __restrict__ blocksum, int* __restrict__ count,
                     long nblk) {
  __shared__ int lds[BLOCK_THREADS];
  int carry = 0;
  for (long base = 0; base < nblk; base += BLOCK_THREADS) {
    const long k = base + threadIdx.x;
    const int v = k < nblk ? blocksum[k] : 0;
    int total;
    const int excl = spo_block_scan(v, lds, total);
    if (k < nblk) blocksum[k] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) *count = carry;
}

__global__ void __launch_bounds__(BLOCK_THREADS) SPO_NOPK
coalesce_emit_kernel(const unsigned int* __restrict__ bitmap,
                     const int* __restrict__ blocksum,
                     int* __restrict__ prefix, int64_t* __restrict__ uniq,
                     long W, long n) {
  __shared__ int lds[BLOCK_THREADS];
  const long nblk = (W + BLOCK_THREADS - 1) / BLOCK_THREADS;
  for (long b = blockIdx.x; b < nblk; b += gridDim.x) {
    const long w = b * BLOCK_THREADS + threadIdx.x;
    unsigned int bits = w < W ? bitmap[w] : 0u;
    int total;
    const int excl = spo_block_scan(__popc(bits), lds, total);
    if (w >= W) continue;  // after the scan: no barrier follows in this trip
    long at = (long)blocksum[b] + excl;
    prefix[w] = (int)at;
    while (bits != 0u) {
      const int bit = __ffs(bits) - 1;
      bits &= bits - 1u;
      if (at < n) uniq[at] = w * 32 + bit;  // at < m <= n by construction
      ++at;
    }
  }
}

__global__ void __launch_bounds__(BLOCK_THREADS) SPO_NOPK
coalesce_count_kernel(const int64_t* __restrict__ ids,
                      const unsigned int* __restrict__ bitmap,
                      const int* __restrict__ prefix, int* __restrict__ slot,
                      int* __restrict__ cnt, long n, long R) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const long id = ids[i];
    if (id < 0 || id >= R) {
      slot[i] = -1;
      continue;
    }
    const long w = id >> 5;
    const unsigned int below = (1u << (id & 31)) - 1u;
    const long s = (long)prefix[w] + __popc(bitmap[w] & below);
    if (s >= n) {  // cannot happen for a zeroed workspace; never index past n
      slot[i] = -1;
      continue;
    }
    slot[i] = (int)s;
    atomicAdd(cnt + s, 1);
  }
}

__global__ void __launch_bounds__(BLOCK_THREADS) SPO_NOPK
coalesce_alloc_kernel(const int* __restrict__ cnt, int* __restrict__ start,
                      int* __restrict__ cursor, const int* __restrict__ count,
                      long n) {
  long m = *count;
  if (m > n) m = n;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < m;
       s += stride)
    start[s] = atomicAdd(cursor, cnt[s]);
}

// After this kernel start[s] is the END of slot s's segment of perm; the
// segment is perm[start[s] - cnt[s], start[s]).
__global__ void __launch_bounds__(BLOCK_THREADS) SPO_NOPK
coalesce_place_kernel(const int64_t* __restrict__ ids,
                      const int* __restrict__ slot, int* __restrict__ start,
                      int* __restrict__ perm, unsigned int* __restrict__ bitmap,
                      long n) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const int s = slot[i];
    if (s < 0) continue;  // id out of range: never marked, nothing to clear
    const int pos = atomicAdd(start + s, 1);
    if (pos >= 0 && pos < n) perm[pos] = (int)i;
    bitmap[ids[i] >> 5] = 0u;  // same-value stores; workspace zero again
  }
}

template <int VEC>
struct SpoAcc {
  float v[VEC];
};

template <int VEC>
__device__ __forceinline__ SPO_NOPK void spo_add_row(
    SpoAcc<VEC>& acc, bool& first, const float* __restrict__ vals, long off,
    float scale) {
  // hipcc fuses a*b + c into an fma by default, in the back end too and for
  // __fmul_rn / __fadd_rn as well; the summation rule needs the product
  // rounded on its own, so it passes through an empty asm the fuser cannot
  // see through
#pragma clang fp contract(off)
  float x[VEC];
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(vals + off);
    x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
  } else {
    x[0] = vals[off];
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    float sv = __fmul_rn(x[k], scale);
    asm volatile("" : "+v"(sv));
    acc.v[k] = first ? sv : __fadd_rn(acc.v[k], sv);
  }
  first = false;
}

template <int VEC>
__global__ void __launch_bounds__(BLOCK_THREADS) SPO_NOPK
coalesce_sum_kernel(const float* __restrict__ vals,
                    const int* __restrict__ slot, const int* __restrict__ cnt,
                    const int* __restrict__ start,
                    const int* __restrict__ perm,
                    const int* __restrict__ count, float* __restrict__ out,
                    int64_t* __restrict__ uniq, long n, long D, int log2_group,
                    float scale) {
  const int group = 1 << log2_group;
  const int rows_per_block = BLOCK_THREADS >> log2_group;
  const int lane = threadIdx.x & (group - 1);
  // bits of this group inside the wave's ballot
  const int wave_lane = threadIdx.x & (WAVE_SIZE - 1);
  const int gshift = wave_lane & ~(group - 1);
  const unsigned long long gmask =
      group == WAVE_SIZE ? ~0ull : ((1ull << group) - 1ull);
  const long chunks = D / VEC;
  long m = *count;
  if (m > n) m = n;
  const long stride = (long)gridDim.x * rows_per_block;
  for (long s = (long)blockIdx.x * rows_per_block + (threadIdx.x >> log2_group);
       s < n; s += stride) {
    const long obase = s * D;
    if (s >= m) {  // pad row
      if (lane == 0) uniq[s] = -1;
      for (long c = lane; c < chunks; c += group) {
        if constexpr (VEC == 4)
          *reinterpret_cast<float4*>(out + obase + c * 4) =
              make_float4(0.f, 0.f, 0.f, 0.f);
        else
          out[obase + c] = 0.f;
      }
      continue;
    }
    const int c_s = cnt[s];
    const int seg = start[s] - c_s;
    // per-lane loads: c*c for the list, n / group for the walk
    const bool by_list = c_s == 1 || (long)c_s * c_s <= (n >> log2_group);
    // group-uniform trip count: the ballots below need every lane of the
    // group, also the ones whose chunk index is past the row
    for (long c0 = 0; c0 < chunks; c0 += group) {
      const long c = c0 + lane;
      const bool live = c < chunks;
      const long coff = c * VEC;
      SpoAcc<VEC> acc;
#pragma unroll
      for (int k = 0; k < VEC; ++k) acc.v[k] = 0.f;
      bool first = true;
      if (by_list) {
        int last = -1;
        for (int t = 0; t < c_s; ++t) {
          int best = 0x7fffffff;
          for (int k = 0; k < c_s; ++k) {
            const int v = perm[seg + k];
            if (v > last && v < best) best = v;
          }
          last = best;
          if (live && best < n)
            spo_add_row<VEC>(acc, first, vals, (long)best * D + coff, scale);
        }
      } else {
        // SPO_WALK_U loads of slot[] in flight per lane, then their
        // ballots in input order
        for (long base = 0; base < n; base += (long)group * SPO_WALK_U) {
          bool hit[SPO_WALK_U];
#pragma unroll
          for (int u = 0; u < SPO_WALK_U; ++u) {
            const long i = base + u * group + lane;
            hit[u] = i < n && slot[i] == (int)s;
          }
#pragma unroll
          for (int u = 0; u < SPO_WALK_U; ++u) {
            unsigned long long mask = (__ballot(hit[u]) >> gshift) & gmask;
            while (mask != 0ull) {
              const int bit = __ffsll((long long)mask) - 1;
              mask &= mask - 1ull;
              if (live)
                spo_add_row<VEC>(acc, first, vals,
                                 (base + u * group + bit) * D + coff, scale);
            }
          }
        }
      }
      if (live) {
        if constexpr (VEC == 4)
          *reinterpret_cast<float4*>(out + obase + coff) =
              make_float4(acc.v[0], acc.v[1], acc.v[2], acc.v[3]);
        else
          out[obase + coff] = acc.v[0];
      }
    }
  }
}
