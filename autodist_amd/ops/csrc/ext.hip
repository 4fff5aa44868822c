// Python bindings for the gfx950 HIP ops (torch extension).
// Launches on the caller's current HIP stream so the engine's comm-stream /
// compute-stream ordering (parallel/engine.py) applies to these kernels too.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "multi_tensor.hip"
#include "bn_ops.hip"
#include "psgd_gemm.hip"
#include "mfma_probe.hip"
#include "attention.hip"
#include "attention_bwd.hip"
#include "ln_ops.hip"
#include "ce_ops.hip"

namespace {

inline hipStream_t cur_stream() {
  return at::cuda::getCurrentCUDAStream().stream();
}

// ---------------------------------------------------------------- fused BN
struct BNGeom {
  long M;
  int C;
  int tx_count, rows_per_blk, grid_c;
};

BNGeom bn_geom(const torch::Tensor& x) {
  TORCH_CHECK(x.dim() == 4, "BN expects NCHW-logical channels_last tensor");
  int C = (int)x.size(1);
  TORCH_CHECK(C % BN_VEC == 0, "C must be a multiple of 8, got ", C);
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "x must be channels_last");
  BNGeom g;
  g.M = x.size(0) * x.size(2) * x.size(3);
  g.C = C;
  g.tx_count = std::min(C / BN_VEC, BLOCK_THREADS);
  g.rows_per_blk = BLOCK_THREADS / g.tx_count;
  g.grid_c = (C / BN_VEC + g.tx_count - 1) / g.tx_count;
  return g;
}

inline int bn_grid_m(const BNGeom& g, long target_blocks) {
  long gm = (g.M + g.rows_per_blk - 1) / g.rows_per_blk;
  long cap = std::max<long>(target_blocks / std::max(g.grid_c, 1), 1);
  return (int)std::min(gm, cap);
}

// Grid of a streaming apply kernel that holds U rows in flight: at most the
// 4096 / grid_c blocks of bn_grid_m, and as many as give every thread a whole
// number of U-row trips (the last blocks fall short where the rows do not
// divide). 2048 x 7 x 7 at batch 512 has 25088 block-rows: 3136 blocks of two
// 4-row trips, where 4096 blocks would run one such trip and two or three
// single rows. Fewer block-rows than U: one block, single rows.
inline int bn_apply_gm(const BNGeom& g, int U) {
  if (U == 1) return bn_grid_m(g, 4096);
  long rows = (g.M + g.rows_per_blk - 1) / g.rows_per_blk;
  long cap = std::max<long>(4096 / std::max(g.grid_c, 1), 1);
  long trips = std::max<long>((rows + U * cap - 1) / (U * cap), 1);
  return (int)((rows + U * trips - 1) / (U * trips));
}

// max partial rows for the two-stage BN reductions (2 blocks per CU).
// NOTE: raising this to 2048 (8 blocks/CU) was MEASURED SLOWER on every
// ResNet shape (tools/bn_microbench.py, 2026-09-14): the reduce stage is
// not occupancy-bound and the larger partial matrix taxes the finalize.
#define BN_GM_MAX 512

inline int bn_reduce_gm(const BNGeom& g) {
  long rows = (g.M + g.rows_per_blk - 1) / g.rows_per_blk;
  long gm = (rows + 31) / 32;
  if (gm < 64) gm = 64;
  if (gm > BN_GM_MAX) gm = BN_GM_MAX;
  if (gm > rows) gm = rows;
  return (int)gm;
}

template <typename T>
T* bn_ptr(const torch::Tensor& t) {
  return reinterpret_cast<T*>(t.data_ptr());
}

template <typename T, bool RELU, bool ADD, bool MASK>
void bn_launch_fwd_apply(dim3 grid, hipStream_t st, const torch::Tensor& x,
                         const torch::Tensor* res, torch::Tensor& y,
                         unsigned char* mask, const float* scale,
                         const float* shift, const BNGeom& g) {
  hipLaunchKernelGGL((bn_fwd_apply_kernel<T, RELU, ADD, MASK>), grid,
                     dim3(BLOCK_THREADS), 0, st, bn_ptr<const T>(x),
                     ADD ? bn_ptr<const T>(*res) : (const T*)nullptr,
                     bn_ptr<T>(y), mask, scale, shift, g.M, g.C);
}

// The statistics stage of every forward entry point: reduce and finalize on
// x. scale / shift point into the workspace and feed the apply kernel that
// the caller launches next on the same stream.
struct BNStats {
  torch::Tensor save_mean, save_rstd;
  const float* scale;
  const float* shift;
  // the workspace, held until the caller has allocated its outputs and
  // launched the apply kernel: when it is a temporary of this call, an
  // output allocated after its release could be given its memory
  torch::Tensor ws;
};

template <typename T>
BNStats bn_fwd_stats(const torch::Tensor& x, const BNGeom& g,
                     const torch::Tensor& weight, const torch::Tensor& bias,
                     torch::Tensor& running_mean, torch::Tensor& running_var,
                     double eps, double momentum,
                     const c10::optional<torch::Tensor>& ws) {
  // ws: persistent per-module workspace [2*BN_GM_MAX + 4, C] fp32:
  //   rows [0, GM)               partial sums (per reduce block)
  //   rows [BN_GM_MAX, BN_GM_MAX+GM) partial sumsq
  //   rows 2*BN_GM_MAX + {0,1}: unused (kept so the layout is unchanged)
  //   rows 2*BN_GM_MAX + {2,3}: scale, shift
  // Everything in ws is dead once this call's apply kernel has run, so a
  // later call on the same module may overwrite it. save_mean / save_rstd
  // and the mask are NOT in ws: autograd keeps them until backward, and a
  // module called twice before backward (shared tower, micro-batches summed
  // into one loss) would otherwise hand the first backward the second
  // call's stats.
  auto fopt = weight.options().dtype(torch::kFloat32);
  torch::Tensor w6 = ws.has_value() ? *ws
      : torch::empty({2 * BN_GM_MAX + 4, (long)g.C}, fopt);
  TORCH_CHECK(w6.size(0) >= 2 * BN_GM_MAX + 4 && w6.size(1) == g.C &&
              w6.is_contiguous());
  float* wp = w6.data_ptr<float>();
  float* partial_sum = wp;
  float* partial_sq = wp + (long)BN_GM_MAX * g.C;
  // fresh allocations: saved for backward (caching-allocator hits, no
  // launch, no fill)
  auto stats = torch::empty({2, (long)g.C}, fopt);
  auto save_mean = stats[0];
  auto save_rstd = stats[1];
  const float* scale = wp + (long)(2 * BN_GM_MAX + 2) * g.C;
  const float* shift = wp + (long)(2 * BN_GM_MAX + 3) * g.C;
  int gm = bn_reduce_gm(g);
  dim3 grid_r(gm, g.grid_c);
  auto st = cur_stream();

  hipLaunchKernelGGL((bn_fwd_reduce_kernel<T>), grid_r, dim3(BLOCK_THREADS),
                     0, st, bn_ptr<const T>(x), partial_sum, partial_sq, g.M,
                     g.C);
  hipLaunchKernelGGL(bn_fwd_finalize_kernel,
                     dim3((g.C + FIN_CH - 1) / FIN_CH),
                     dim3(FIN_CH * FIN_LANES), 0, st, partial_sum, partial_sq,
                     gm, weight.data_ptr<float>(), bias.data_ptr<float>(),
                     running_mean.data_ptr<float>(),
                     running_var.data_ptr<float>(),
                     save_mean.data_ptr<float>(), save_rstd.data_ptr<float>(),
                     const_cast<float*>(scale), const_cast<float*>(shift),
                     g.M, g.C, (float)eps, (float)momentum);
  return {save_mean, save_rstd, scale, shift, w6};
}

// with_mask: also return the bit-packed ReLU mask of y ([M, C/8] uint8, see
// bn_fwd_apply_kernel), which bn_bwd_mask takes in place of y.
template <typename T>
std::vector<torch::Tensor> bn_fwd_impl(
    const torch::Tensor& x, const torch::Tensor& weight,
    const torch::Tensor& bias, torch::Tensor& running_mean,
    torch::Tensor& running_var, const c10::optional<torch::Tensor>& res,
    double eps, double momentum, bool relu,
    const c10::optional<torch::Tensor>& ws, bool with_mask) {
  TORCH_CHECK(!with_mask || relu, "the mask is the ReLU mask: relu must be set");
  auto g = bn_geom(x);
  BNStats s = bn_fwd_stats<T>(x, g, weight, bias, running_mean, running_var,
                              eps, momentum, ws);
  auto save_mean = s.save_mean, save_rstd = s.save_rstd;
  const float* scale = s.scale;
  const float* shift = s.shift;
  torch::Tensor mask;
  if (with_mask)
    mask = torch::empty({g.M, (long)(g.C / BN_VEC)},
                        x.options().dtype(torch::kUInt8));
  unsigned char* mp = with_mask ? mask.data_ptr<unsigned char>() : nullptr;
  auto y = torch::empty_like(x);
  dim3 grid_a(bn_apply_gm(g, BN_APPLY_FWD_U), g.grid_c);
  auto st = cur_stream();
  const torch::Tensor* rp = res.has_value() ? &*res : nullptr;
#define BN_FWD_APPLY(RELU, ADD, MASK)                                        \
  bn_launch_fwd_apply<T, RELU, ADD, MASK>(grid_a, st, x, rp, y, mp, scale,  \
                                          shift, g)
  if (rp) {
    if (with_mask) BN_FWD_APPLY(true, true, true);
    else if (relu) BN_FWD_APPLY(true, true, false);
    else BN_FWD_APPLY(false, true, false);
  } else {
    if (with_mask) BN_FWD_APPLY(true, false, true);
    else if (relu) BN_FWD_APPLY(true, false, false);
    else BN_FWD_APPLY(false, false, false);
  }
#undef BN_FWD_APPLY
  if (with_mask) return {y, save_mean, save_rstd, mask};
  return {y, save_mean, save_rstd};
}

std::vector<torch::Tensor> bn_fwd_dispatch(
    const torch::Tensor& x, const torch::Tensor& weight,
    const torch::Tensor& bias, torch::Tensor& running_mean,
    torch::Tensor& running_var, const c10::optional<torch::Tensor>& res,
    double eps, double momentum, bool relu,
    const c10::optional<torch::Tensor>& ws, bool with_mask) {
  if (x.scalar_type() == torch::kBFloat16)
    return bn_fwd_impl<__hip_bfloat16>(x, weight, bias, running_mean,
                                       running_var, res, eps, momentum, relu,
                                       ws, with_mask);
  TORCH_CHECK(x.scalar_type() == torch::kFloat32);
  return bn_fwd_impl<float>(x, weight, bias, running_mean, running_var, res,
                            eps, momentum, relu, ws, with_mask);
}

std::vector<torch::Tensor> bn_fwd_train(torch::Tensor x, torch::Tensor weight,
                                        torch::Tensor bias,
                                        torch::Tensor running_mean,
                                        torch::Tensor running_var,
                                        c10::optional<torch::Tensor> res,
                                        double eps, double momentum,
                                        bool relu,
                                        c10::optional<torch::Tensor> ws) {
  return bn_fwd_dispatch(x, weight, bias, running_mean, running_var, res, eps,
                         momentum, relu, ws, false);
}

// -> (y, save_mean, save_rstd, mask); relu must be true
std::vector<torch::Tensor> bn_fwd_train_mask(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor running_mean, torch::Tensor running_var,
    c10::optional<torch::Tensor> res, double eps, double momentum, bool relu,
    c10::optional<torch::Tensor> ws) {
  return bn_fwd_dispatch(x, weight, bias, running_mean, running_var, res, eps,
                         momentum, relu, ws, true);
}

// ------------------------------------------- bn + relu + 3x3/s2/p1 max-pool
inline BNPool bn_pool_geom(const torch::Tensor& x, const BNGeom& g) {
  BNPool p;
  p.amax = nullptr;
  p.H = (int)x.size(2);
  p.W = (int)x.size(3);
  p.Ho = (p.H - 1) / 2 + 1;
  p.Wo = (p.W - 1) / 2 + 1;
  // the kernels index pixels, and the pooled tensor's elements, in 32 bits
  TORCH_CHECK(g.M < (1L << 31), "bn pool: N*H*W must be below 2^31");
  TORCH_CHECK(x.size(0) * (long)p.Ho * p.Wo * g.C < (1L << 31),
              "bn pool: the pooled tensor must hold fewer than 2^31 elements");
  return p;
}

// -> (pooled y, save_mean, save_rstd, argmax [N*Ho*Wo, C/8] int32)
template <typename T>
std::vector<torch::Tensor> bn_fwd_pool_impl(
    const torch::Tensor& x, const torch::Tensor& weight,
    const torch::Tensor& bias, torch::Tensor& running_mean,
    torch::Tensor& running_var, double eps, double momentum,
    const c10::optional<torch::Tensor>& ws) {
  auto g = bn_geom(x);
  BNPool p = bn_pool_geom(x, g);
  BNStats s = bn_fwd_stats<T>(x, g, weight, bias, running_mean, running_var,
                              eps, momentum, ws);
  BNGeom go = g;
  go.M = x.size(0) * (long)p.Ho * p.Wo;
  auto y = torch::empty({x.size(0), x.size(1), (long)p.Ho, (long)p.Wo},
                        x.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto amax = torch::empty({go.M, (long)(g.C / BN_VEC)},
                           x.options().dtype(torch::kInt32));
  dim3 grid_a(bn_grid_m(go, 4096), g.grid_c);
  hipLaunchKernelGGL((bn_fwd_pool_apply_kernel<T>), grid_a,
                     dim3(BLOCK_THREADS), 0, cur_stream(), bn_ptr<const T>(x),
                     bn_ptr<T>(y), bn_ptr<unsigned>(amax), s.scale, s.shift,
                     p, go.M, g.C);
  return {y, s.save_mean, s.save_rstd, amax};
}

std::vector<torch::Tensor> bn_fwd_train_pool(
    torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
    torch::Tensor running_mean, torch::Tensor running_var, double eps,
    double momentum, c10::optional<torch::Tensor> ws) {
  if (x.scalar_type() == torch::kBFloat16)
    return bn_fwd_pool_impl<__hip_bfloat16>(x, weight, bias, running_mean,
                                            running_var, eps, momentum, ws);
  TORCH_CHECK(x.scalar_type() == torch::kFloat32);
  return bn_fwd_pool_impl<float>(x, weight, bias, running_mean, running_var,
                                 eps, momentum, ws);
}

// ------------------------------------ block tail: relu(bn3(z) + bn_ds(zd))
// -> (y, mask, save_mean, save_rstd, save_mean_d, save_rstd_d). Each BN runs
// its statistics in its own workspace; one apply kernel joins them. Backward
// is bn_bwd_mask on (z, bn3 stats) and on (zd, downsample stats), both with
// the dy and the mask of y.
template <typename T>
std::vector<torch::Tensor> bn_fwd_add_bn_impl(
    const torch::Tensor& z, const torch::Tensor& zd,
    const torch::Tensor& weight, const torch::Tensor& bias,
    torch::Tensor& running_mean, torch::Tensor& running_var, double eps,
    double momentum, const c10::optional<torch::Tensor>& ws,
    const torch::Tensor& weight_d, const torch::Tensor& bias_d,
    torch::Tensor& running_mean_d, torch::Tensor& running_var_d, double eps_d,
    double momentum_d, const c10::optional<torch::Tensor>& ws_d) {
  auto g = bn_geom(z);
  auto gd = bn_geom(zd);
  TORCH_CHECK(zd.sizes() == z.sizes() && zd.scalar_type() == z.scalar_type() &&
                  zd.device() == z.device() && gd.M == g.M,
              "bn_fwd_train_add_bn: z and zd must agree in shape and dtype");
  TORCH_CHECK(!ws.has_value() || !ws_d.has_value() ||
                  ws->data_ptr() != ws_d->data_ptr(),
              "bn_fwd_train_add_bn: the two BNs need workspaces of their own");
  BNStats s = bn_fwd_stats<T>(z, g, weight, bias, running_mean, running_var,
                              eps, momentum, ws);
  BNStats sd = bn_fwd_stats<T>(zd, gd, weight_d, bias_d, running_mean_d,
                               running_var_d, eps_d, momentum_d, ws_d);
  auto y = torch::empty_like(z);
  auto mask = torch::empty({g.M, (long)(g.C / BN_VEC)},
                           z.options().dtype(torch::kUInt8));
  dim3 grid_a(bn_apply_gm(g, BN_APPLY_FWD_U), g.grid_c);
  hipLaunchKernelGGL((bn_fwd_apply_add_bn_kernel<T>), grid_a,
                     dim3(BLOCK_THREADS), 0, cur_stream(), bn_ptr<const T>(z),
                     bn_ptr<const T>(zd), bn_ptr<T>(y),
                     mask.data_ptr<unsigned char>(), s.scale, s.shift,
                     sd.scale, sd.shift, g.M, g.C);
  return {y, mask, s.save_mean, s.save_rstd, sd.save_mean, sd.save_rstd};
}

std::vector<torch::Tensor> bn_fwd_train_add_bn(
    torch::Tensor z, torch::Tensor zd, torch::Tensor weight,
    torch::Tensor bias, torch::Tensor running_mean, torch::Tensor running_var,
    double eps, double momentum, c10::optional<torch::Tensor> ws,
    torch::Tensor weight_d, torch::Tensor bias_d, torch::Tensor running_mean_d,
    torch::Tensor running_var_d, double eps_d, double momentum_d,
    c10::optional<torch::Tensor> ws_d) {
  if (z.scalar_type() == torch::kBFloat16)
    return bn_fwd_add_bn_impl<__hip_bfloat16>(
        z, zd, weight, bias, running_mean, running_var, eps, momentum, ws,
        weight_d, bias_d, running_mean_d, running_var_d, eps_d, momentum_d,
        ws_d);
  TORCH_CHECK(z.scalar_type() == torch::kFloat32);
  return bn_fwd_add_bn_impl<float>(
      z, zd, weight, bias, running_mean, running_var, eps, momentum, ws,
      weight_d, bias_d, running_mean_d, running_var_d, eps_d, momentum_d,
      ws_d);
}

// RELU: BN_RELU_NONE / BN_RELU_Y (yq is y, same dtype and layout as x) /
// BN_RELU_MASK (yq is the forward's packed mask).
template <typename T, int RELU>
std::vector<torch::Tensor> bn_bwd_impl(
    const torch::Tensor& x, const torch::Tensor& dy, const torch::Tensor& yq,
    const torch::Tensor& save_mean, const torch::Tensor& save_rstd,
    const torch::Tensor& weight, bool need_dres,
    const c10::optional<torch::Tensor>& ws) {
  // ws rows: [0,GM) partial_dz, [BN_GM_MAX, BN_GM_MAX+GM) partial_dzxh,
  //          2*BN_GM_MAX + {0,1,2}: k1, k2, k3.
  auto g = bn_geom(x);
  auto fopt = weight.options().dtype(torch::kFloat32);
  torch::Tensor w5 = ws.has_value() ? *ws
      : torch::empty({2 * BN_GM_MAX + 3, (long)g.C}, fopt);
  TORCH_CHECK(w5.size(0) >= 2 * BN_GM_MAX + 3 && w5.size(1) == g.C &&
              w5.is_contiguous());
  const T* yp = nullptr;
  const unsigned char* mp = nullptr;
  if (RELU == BN_RELU_MASK) {
    TORCH_CHECK(yq.scalar_type() == torch::kUInt8 && yq.is_contiguous() &&
                    yq.dim() == 2 && yq.size(0) == g.M &&
                    yq.size(1) == g.C / BN_VEC && yq.device() == x.device(),
                "mask must be the [M, C/8] uint8 tensor of bn_fwd_train_mask");
    mp = yq.data_ptr<unsigned char>();
  } else {
    yp = bn_ptr<const T>(yq);
  }
  float* wp = w5.data_ptr<float>();
  float* partial_dz = wp;
  float* partial_dzxh = wp + (long)BN_GM_MAX * g.C;
  float* k1 = wp + (long)(2 * BN_GM_MAX + 0) * g.C;
  float* k2 = wp + (long)(2 * BN_GM_MAX + 1) * g.C;
  float* k3 = wp + (long)(2 * BN_GM_MAX + 2) * g.C;
  // fresh allocations: returned to autograd as parameter gradients
  auto dweight = torch::empty({g.C}, fopt);
  auto dbias = torch::empty({g.C}, fopt);
  auto dx = torch::empty_like(x);
  torch::Tensor dres;
  if (need_dres) dres = torch::empty_like(x);
  dim3 block(BLOCK_THREADS);
  int gm = bn_reduce_gm(g);
  dim3 grid_r(gm, g.grid_c);
  dim3 grid_a(bn_apply_gm(g, BN_APPLY_BWD_U), g.grid_c);
  auto st = cur_stream();
  const float* sm = save_mean.data_ptr<float>();
  const float* sr = save_rstd.data_ptr<float>();

  hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, RELU>), grid_r, block, 0, st,
                     bn_ptr<const T>(x), bn_ptr<const T>(dy), yp, mp, sm, sr,
                     partial_dz, partial_dzxh, g.M, g.C, BNPool{});
  hipLaunchKernelGGL(bn_bwd_finalize_kernel,
                     dim3((g.C + FIN_CH - 1) / FIN_CH),
                     dim3(FIN_CH * FIN_LANES), 0, st, partial_dz,
                     partial_dzxh, gm, weight.data_ptr<float>(), sr, k1, k2,
                     k3, dweight.data_ptr<float>(), dbias.data_ptr<float>(),
                     g.M, g.C);
  if (need_dres)
    hipLaunchKernelGGL((bn_bwd_apply_kernel<T, RELU, true>), grid_a, block, 0,
                       st, bn_ptr<const T>(x), bn_ptr<const T>(dy), yp, mp,
                       sm, sr, k1, k2, k3, bn_ptr<T>(dx), bn_ptr<T>(dres),
                       g.M, g.C, BNPool{});
  else
    hipLaunchKernelGGL((bn_bwd_apply_kernel<T, RELU, false>), grid_a, block,
                       0, st, bn_ptr<const T>(x), bn_ptr<const T>(dy), yp, mp,
                       sm, sr, k1, k2, k3, bn_ptr<T>(dx), (T*)nullptr, g.M,
                       g.C, BNPool{});
  std::vector<torch::Tensor> out = {dx, dweight, dbias};
  if (need_dres) out.push_back(dres);
  return out;
}

template <int RELU>
std::vector<torch::Tensor> bn_bwd_dispatch(
    const torch::Tensor& x, const torch::Tensor& dy, const torch::Tensor& yq,
    const torch::Tensor& save_mean, const torch::Tensor& save_rstd,
    const torch::Tensor& weight, bool need_dres,
    const c10::optional<torch::Tensor>& ws) {
  if (x.scalar_type() == torch::kBFloat16)
    return bn_bwd_impl<__hip_bfloat16, RELU>(x, dy, yq, save_mean, save_rstd,
                                             weight, need_dres, ws);
  TORCH_CHECK(x.scalar_type() == torch::kFloat32);
  return bn_bwd_impl<float, RELU>(x, dy, yq, save_mean, save_rstd, weight,
                                  need_dres, ws);
}

std::vector<torch::Tensor> bn_bwd(torch::Tensor x, torch::Tensor dy,
                                  torch::Tensor y, torch::Tensor save_mean,
                                  torch::Tensor save_rstd,
                                  torch::Tensor weight, bool relu,
                                  bool need_dres,
                                  c10::optional<torch::Tensor> ws) {
  if (relu)
    return bn_bwd_dispatch<BN_RELU_Y>(x, dy, y, save_mean, save_rstd, weight,
                                      need_dres, ws);
  return bn_bwd_dispatch<BN_RELU_NONE>(x, dy, y, save_mean, save_rstd, weight,
                                       need_dres, ws);
}

// bn_bwd with the packed mask of bn_fwd_train_mask in place of y
std::vector<torch::Tensor> bn_bwd_mask(torch::Tensor x, torch::Tensor dy,
                                       torch::Tensor mask,
                                       torch::Tensor save_mean,
                                       torch::Tensor save_rstd,
                                       torch::Tensor weight, bool relu,
                                       bool need_dres,
                                       c10::optional<torch::Tensor> ws) {
  TORCH_CHECK(relu, "the mask is the ReLU mask: relu must be set");
  return bn_bwd_dispatch<BN_RELU_MASK>(x, dy, mask, save_mean, save_rstd,
                                       weight, need_dres, ws);
}

// bn_bwd_mask for a dy that arrives as two addends: the join reduce forms
// dz = mask ? T(dy_a + dy_b) : 0 and stores it, the finalize is the usual
// one, and the plain apply runs on dy = dz. Returns (dx, dweight, dbias, dz);
// dz is what bn_bwd_mask(need_dres) returns as dres for dy = dy_a + dy_b.
template <typename T>
std::vector<torch::Tensor> bn_bwd_mask_join_impl(
    const torch::Tensor& x, const torch::Tensor& dy_a,
    const torch::Tensor& dy_b, const torch::Tensor& mask,
    const torch::Tensor& save_mean, const torch::Tensor& save_rstd,
    const torch::Tensor& weight, const c10::optional<torch::Tensor>& ws) {
  // ws rows as in bn_bwd_impl
  auto g = bn_geom(x);
  for (const torch::Tensor* d : {&dy_a, &dy_b})
    TORCH_CHECK(d->sizes() == x.sizes() &&
                    d->scalar_type() == x.scalar_type() &&
                    d->device() == x.device() &&
                    d->is_contiguous(at::MemoryFormat::ChannelsLast),
                "bn_bwd_mask_join: dy_a and dy_b must match x in shape, "
                "dtype, device and channels_last layout");
  auto fopt = weight.options().dtype(torch::kFloat32);
  torch::Tensor w5 = ws.has_value() ? *ws
      : torch::empty({2 * BN_GM_MAX + 3, (long)g.C}, fopt);
  TORCH_CHECK(w5.size(0) >= 2 * BN_GM_MAX + 3 && w5.size(1) == g.C &&
              w5.is_contiguous());
  TORCH_CHECK(mask.scalar_type() == torch::kUInt8 && mask.is_contiguous() &&
                  mask.dim() == 2 && mask.size(0) == g.M &&
                  mask.size(1) == g.C / BN_VEC && mask.device() == x.device(),
              "mask must be the [M, C/8] uint8 tensor of bn_fwd_train_mask");
  const unsigned char* mp = mask.data_ptr<unsigned char>();
  float* wp = w5.data_ptr<float>();
  float* partial_dz = wp;
  float* partial_dzxh = wp + (long)BN_GM_MAX * g.C;
  float* k1 = wp + (long)(2 * BN_GM_MAX + 0) * g.C;
  float* k2 = wp + (long)(2 * BN_GM_MAX + 1) * g.C;
  float* k3 = wp + (long)(2 * BN_GM_MAX + 2) * g.C;
  auto dweight = torch::empty({g.C}, fopt);
  auto dbias = torch::empty({g.C}, fopt);
  auto dx = torch::empty_like(x);
  auto dz = torch::empty_like(x);
  dim3 block(BLOCK_THREADS);
  int gm = bn_reduce_gm(g);
  dim3 grid_r(gm, g.grid_c);
  dim3 grid_a(bn_apply_gm(g, BN_APPLY_BWD_U), g.grid_c);
  auto st = cur_stream();
  const float* sm = save_mean.data_ptr<float>();
  const float* sr = save_rstd.data_ptr<float>();

  hipLaunchKernelGGL((bn_bwd_reduce_join_kernel<T>), grid_r, block, 0, st,
                     bn_ptr<const T>(x), bn_ptr<const T>(dy_a),
                     bn_ptr<const T>(dy_b), mp, sm, sr, partial_dz,
                     partial_dzxh, bn_ptr<T>(dz), g.M, g.C);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel,
                     dim3((g.C + FIN_CH - 1) / FIN_CH),
                     dim3(FIN_CH * FIN_LANES), 0, st, partial_dz,
                     partial_dzxh, gm, weight.data_ptr<float>(), sr, k1, k2,
                     k3, dweight.data_ptr<float>(), dbias.data_ptr<float>(),
                     g.M, g.C);
  hipLaunchKernelGGL((bn_bwd_apply_kernel<T, BN_RELU_NONE, false>), grid_a,
                     block, 0, st, bn_ptr<const T>(x), bn_ptr<const T>(dz),
                     (const T*)nullptr, (const unsigned char*)nullptr, sm, sr,
                     k1, k2, k3, bn_ptr<T>(dx), (T*)nullptr, g.M, g.C,
                     BNPool{});
  return {dx, dweight, dbias, dz};
}

std::vector<torch::Tensor> bn_bwd_mask_join(
    torch::Tensor x, torch::Tensor dy_a, torch::Tensor dy_b,
    torch::Tensor mask, torch::Tensor save_mean, torch::Tensor save_rstd,
    torch::Tensor weight, c10::optional<torch::Tensor> ws) {
  if (x.scalar_type() == torch::kBFloat16)
    return bn_bwd_mask_join_impl<__hip_bfloat16>(x, dy_a, dy_b, mask,
                                                 save_mean, save_rstd, weight,
                                                 ws);
  TORCH_CHECK(x.scalar_type() == torch::kFloat32);
  return bn_bwd_mask_join_impl<float>(x, dy_a, dy_b, mask, save_mean,
                                      save_rstd, weight, ws);
}

// Backward of relu(bn(z) + bn_d(zd)) for a dy that arrives as two addends:
// bn_bwd_mask_join on z followed by the mask-less bn_bwd on (zd, dz), with
// the two reduces and the two applies each done in one pass (10 tensor passes
// where those run 12). Every output is what that pair of calls returns.
// -> (dx, dweight, dbias, dz, dx_d, dweight_d, dbias_d)
template <typename T>
std::vector<torch::Tensor> bn_bwd_mask_join_bn_impl(
    const torch::Tensor& z, const torch::Tensor& dy_a,
    const torch::Tensor& dy_b, const torch::Tensor& mask,
    const torch::Tensor& save_mean, const torch::Tensor& save_rstd,
    const torch::Tensor& weight, const c10::optional<torch::Tensor>& ws,
    const torch::Tensor& zd, const torch::Tensor& save_mean_d,
    const torch::Tensor& save_rstd_d, const torch::Tensor& weight_d,
    const c10::optional<torch::Tensor>& ws_d) {
  auto g = bn_geom(z);
  auto gd = bn_geom(zd);
  TORCH_CHECK(gd.M == g.M && gd.C == g.C &&
                  zd.scalar_type() == z.scalar_type() &&
                  zd.device() == z.device(),
              "bn_bwd_mask_join: z and zd must agree in shape and dtype");
  for (const torch::Tensor* d : {&dy_a, &dy_b})
    TORCH_CHECK(d->sizes() == z.sizes() &&
                    d->scalar_type() == z.scalar_type() &&
                    d->device() == z.device() &&
                    d->is_contiguous(at::MemoryFormat::ChannelsLast),
                "bn_bwd_mask_join: dy_a and dy_b must match x in shape, "
                "dtype, device and channels_last layout");
  TORCH_CHECK(!(ws.has_value() && ws_d.has_value()) ||
                  ws->data_ptr() != ws_d->data_ptr(),
              "bn_bwd_mask_join: the two BNs need workspaces of their own");
  // ws rows as in bn_bwd_impl, one workspace per branch; the d branch's
  // partial_dz rows stay unused: sum dz is taken once, into ws
  auto fopt = weight.options().dtype(torch::kFloat32);
  torch::Tensor w5 = ws.has_value() ? *ws
      : torch::empty({2 * BN_GM_MAX + 3, (long)g.C}, fopt);
  torch::Tensor w5d = ws_d.has_value() ? *ws_d
      : torch::empty({2 * BN_GM_MAX + 3, (long)g.C}, fopt);
  for (const torch::Tensor* w : {&w5, &w5d})
    TORCH_CHECK(w->size(0) >= 2 * BN_GM_MAX + 3 && w->size(1) == g.C &&
                w->is_contiguous());
  TORCH_CHECK(mask.scalar_type() == torch::kUInt8 && mask.is_contiguous() &&
                  mask.dim() == 2 && mask.size(0) == g.M &&
                  mask.size(1) == g.C / BN_VEC && mask.device() == z.device(),
              "mask must be the [M, C/8] uint8 tensor of bn_fwd_train_mask");
  const unsigned char* mp = mask.data_ptr<unsigned char>();
  float* wp = w5.data_ptr<float>();
  float* wpd = w5d.data_ptr<float>();
  float* partial_dz = wp;
  float* partial_dzxh = wp + (long)BN_GM_MAX * g.C;
  float* partial_dzxh_d = wpd + (long)BN_GM_MAX * g.C;
  float* k1 = wp + (long)(2 * BN_GM_MAX + 0) * g.C;
  float* k2 = wp + (long)(2 * BN_GM_MAX + 1) * g.C;
  float* k3 = wp + (long)(2 * BN_GM_MAX + 2) * g.C;
  float* k1_d = wpd + (long)(2 * BN_GM_MAX + 0) * g.C;
  float* k2_d = wpd + (long)(2 * BN_GM_MAX + 1) * g.C;
  float* k3_d = wpd + (long)(2 * BN_GM_MAX + 2) * g.C;
  auto dweight = torch::empty({g.C}, fopt);
  auto dbias = torch::empty({g.C}, fopt);
  auto dweight_d = torch::empty({g.C}, fopt);
  auto dbias_d = torch::empty({g.C}, fopt);
  auto dx = torch::empty_like(z);
  auto dx_d = torch::empty_like(zd);
  auto dz = torch::empty_like(z);
  dim3 block(BLOCK_THREADS);
  int gm = bn_reduce_gm(g);
  dim3 grid_r(gm, g.grid_c);
  dim3 grid_a(bn_apply_gm(g, BN_APPLY2_U), g.grid_c);
  dim3 grid_f((g.C + FIN_CH - 1) / FIN_CH), block_f(FIN_CH * FIN_LANES);
  auto st = cur_stream();
  const float* sm = save_mean.data_ptr<float>();
  const float* sr = save_rstd.data_ptr<float>();
  const float* smd = save_mean_d.data_ptr<float>();
  const float* srd = save_rstd_d.data_ptr<float>();

  hipLaunchKernelGGL((bn_bwd_reduce_join2_kernel<T>), grid_r, block, 0, st,
                     bn_ptr<const T>(z), bn_ptr<const T>(zd),
                     bn_ptr<const T>(dy_a), bn_ptr<const T>(dy_b), mp, sm, sr,
                     smd, srd, partial_dz, partial_dzxh, partial_dzxh_d,
                     bn_ptr<T>(dz), g.M, g.C);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, grid_f, block_f, 0, st,
                     partial_dz, partial_dzxh, gm, weight.data_ptr<float>(),
                     sr, k1, k2, k3, dweight.data_ptr<float>(),
                     dbias.data_ptr<float>(), g.M, g.C);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, grid_f, block_f, 0, st,
                     partial_dz, partial_dzxh_d, gm,
                     weight_d.data_ptr<float>(), srd, k1_d, k2_d, k3_d,
                     dweight_d.data_ptr<float>(), dbias_d.data_ptr<float>(),
                     g.M, g.C);
  hipLaunchKernelGGL((bn_bwd_apply2_kernel<T>), grid_a, block, 0, st,
                     bn_ptr<const T>(z), bn_ptr<const T>(zd),
                     bn_ptr<const T>(dz), sm, sr, smd, srd, k1, k2, k3, k1_d,
                     k3_d, bn_ptr<T>(dx), bn_ptr<T>(dx_d), g.M, g.C);
  return {dx, dweight, dbias, dz, dx_d, dweight_d, dbias_d};
}

// Bound as a second signature of bn_bwd_mask_join: the arguments of the
// one-BN call, then the downsample branch's zd, statistics, weight and ws.
std::vector<torch::Tensor> bn_bwd_mask_join_bn(
    torch::Tensor z, torch::Tensor dy_a, torch::Tensor dy_b,
    torch::Tensor mask, torch::Tensor save_mean, torch::Tensor save_rstd,
    torch::Tensor weight, c10::optional<torch::Tensor> ws, torch::Tensor zd,
    torch::Tensor save_mean_d, torch::Tensor save_rstd_d,
    torch::Tensor weight_d, c10::optional<torch::Tensor> ws_d) {
  if (z.scalar_type() == torch::kBFloat16)
    return bn_bwd_mask_join_bn_impl<__hip_bfloat16>(
        z, dy_a, dy_b, mask, save_mean, save_rstd, weight, ws, zd,
        save_mean_d, save_rstd_d, weight_d, ws_d);
  TORCH_CHECK(z.scalar_type() == torch::kFloat32);
  return bn_bwd_mask_join_bn_impl<float>(z, dy_a, dy_b, mask, save_mean,
                                         save_rstd, weight, ws, zd,
                                         save_mean_d, save_rstd_d, weight_d,
                                         ws_d);
}

// bn_bwd for bn_fwd_train_pool: dy is the pooled dy, argmax the forward's
// argmax words; the kernels gather dz through them (BN_RELU_POOL).
// -> (dx, dweight, dbias)
template <typename T>
std::vector<torch::Tensor> bn_bwd_pool_impl(
    const torch::Tensor& x, const torch::Tensor& dy,
    const torch::Tensor& argmax, const torch::Tensor& save_mean,
    const torch::Tensor& save_rstd, const torch::Tensor& weight,
    const c10::optional<torch::Tensor>& ws) {
  auto g = bn_geom(x);
  BNPool p = bn_pool_geom(x, g);
  const long Mo = x.size(0) * (long)p.Ho * p.Wo;
  TORCH_CHECK(dy.dim() == 4 && dy.size(0) == x.size(0) && dy.size(1) == g.C &&
                  dy.size(2) == p.Ho && dy.size(3) == p.Wo &&
                  dy.scalar_type() == x.scalar_type() &&
                  dy.device() == x.device() &&
                  dy.is_contiguous(at::MemoryFormat::ChannelsLast),
              "dy must be the channels_last [N, C, Ho, Wo] gradient of the "
              "pooled y");
  TORCH_CHECK(argmax.scalar_type() == torch::kInt32 && argmax.is_contiguous() &&
                  argmax.dim() == 2 && argmax.size(0) == Mo &&
                  argmax.size(1) == g.C / BN_VEC &&
                  argmax.device() == x.device(),
              "argmax must be the [N*Ho*Wo, C/8] int32 tensor of "
              "bn_fwd_train_pool");
  p.amax = bn_ptr<const unsigned>(argmax);
  auto fopt = weight.options().dtype(torch::kFloat32);
  torch::Tensor w5 = ws.has_value() ? *ws
      : torch::empty({2 * BN_GM_MAX + 3, (long)g.C}, fopt);
  TORCH_CHECK(w5.size(0) >= 2 * BN_GM_MAX + 3 && w5.size(1) == g.C &&
              w5.is_contiguous());
  float* wp = w5.data_ptr<float>();
  float* partial_dz = wp;
  float* partial_dzxh = wp + (long)BN_GM_MAX * g.C;
  float* k1 = wp + (long)(2 * BN_GM_MAX + 0) * g.C;
  float* k2 = wp + (long)(2 * BN_GM_MAX + 1) * g.C;
  float* k3 = wp + (long)(2 * BN_GM_MAX + 2) * g.C;
  auto dweight = torch::empty({g.C}, fopt);
  auto dbias = torch::empty({g.C}, fopt);
  auto dx = torch::empty_like(x);
  dim3 block(BLOCK_THREADS);
  int gm = bn_reduce_gm(g);
  dim3 grid_r(gm, g.grid_c);
  dim3 grid_a(bn_grid_m(g, 4096), g.grid_c);
  auto st = cur_stream();
  const float* sm = save_mean.data_ptr<float>();
  const float* sr = save_rstd.data_ptr<float>();
  hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, BN_RELU_POOL>), grid_r, block, 0,
                     st, bn_ptr<const T>(x), bn_ptr<const T>(dy),
                     (const T*)nullptr, (const unsigned char*)nullptr, sm, sr,
                     partial_dz, partial_dzxh, g.M, g.C, p);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel,
                     dim3((g.C + FIN_CH - 1) / FIN_CH),
                     dim3(FIN_CH * FIN_LANES), 0, st, partial_dz,
                     partial_dzxh, gm, weight.data_ptr<float>(), sr, k1, k2,
                     k3, dweight.data_ptr<float>(), dbias.data_ptr<float>(),
                     g.M, g.C);
  hipLaunchKernelGGL((bn_bwd_apply_kernel<T, BN_RELU_POOL, false>), grid_a,
                     block, 0, st, bn_ptr<const T>(x), bn_ptr<const T>(dy),
                     (const T*)nullptr, (const unsigned char*)nullptr, sm, sr,
                     k1, k2, k3, bn_ptr<T>(dx), (T*)nullptr, g.M, g.C, p);
  return {dx, dweight, dbias};
}

std::vector<torch::Tensor> bn_bwd_pool(torch::Tensor x, torch::Tensor dy,
                                       torch::Tensor argmax,
                                       torch::Tensor save_mean,
                                       torch::Tensor save_rstd,
                                       torch::Tensor weight,
                                       c10::optional<torch::Tensor> ws) {
  if (x.scalar_type() == torch::kBFloat16)
    return bn_bwd_pool_impl<__hip_bfloat16>(x, dy, argmax, save_mean,
                                            save_rstd, weight, ws);
  TORCH_CHECK(x.scalar_type() == torch::kFloat32);
  return bn_bwd_pool_impl<float>(x, dy, argmax, save_mean, save_rstd, weight,
                                 ws);
}

void check_f32_flat(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
}

// The launchers are shared by the fp32-gradient entry points and by the
// *_wire entry points, whose gradient is the bf16 wire shard of the sharded
// dense schedule (multi_tensor.hip, "gradient stream").
template <typename GT>
void launch_fused_sgd(torch::Tensor& p, const GT* g,
                      c10::optional<torch::Tensor>& buf, double lr,
                      double momentum, double dampening, double weight_decay,
                      bool nesterov, bool first_step, bool maximize) {
  long n = p.numel();
  dim3 grid(grid_for(n)), block(BLOCK_THREADS);
  if (buf.has_value()) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(fused_sgd_kernel<true, GT>), grid,
                       block, 0, cur_stream(), p.data_ptr<float>(), g,
                       buf->data_ptr<float>(), n, (float)lr, (float)momentum,
                       (float)(1.0 - dampening), (float)weight_decay, nesterov,
                       first_step, maximize);
  } else {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(fused_sgd_kernel<false, GT>), grid,
                       block, 0, cur_stream(), p.data_ptr<float>(), g,
                       nullptr, n, (float)lr, (float)momentum,
                       (float)(1.0 - dampening), (float)weight_decay, nesterov,
                       first_step, maximize);
  }
}

template <typename GT>
void launch_fused_adam(torch::Tensor& p, const GT* g, torch::Tensor& m,
                       torch::Tensor& v, double lr, double beta1, double beta2,
                       double eps, double weight_decay, bool adamw, double bc1,
                       double sqrt_bc2, bool maximize) {
  long n = p.numel();
  hipLaunchKernelGGL(HIP_KERNEL_NAME(fused_adam_kernel<GT>),
                     dim3(grid_for(n)), dim3(BLOCK_THREADS), 0, cur_stream(),
                     p.data_ptr<float>(), g, m.data_ptr<float>(),
                     v.data_ptr<float>(), n, (float)lr, (float)beta1,
                     (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2),
                     (float)eps, (float)weight_decay, adamw, (float)bc1,
                     (float)sqrt_bc2, maximize);
}

template <typename GT>
void launch_fused_adagrad(torch::Tensor& p, const GT* g, torch::Tensor& sum,
                          double clr, double eps, double weight_decay,
                          bool maximize) {
  long n = p.numel();
  hipLaunchKernelGGL(HIP_KERNEL_NAME(fused_adagrad_kernel<GT>),
                     dim3(grid_for(n)), dim3(BLOCK_THREADS), 0, cur_stream(),
                     p.data_ptr<float>(), g, sum.data_ptr<float>(), n,
                     (float)clr, (float)eps, (float)weight_decay, maximize);
}

void fused_sgd(torch::Tensor p, torch::Tensor g,
               c10::optional<torch::Tensor> buf, double lr, double momentum,
               double dampening, double weight_decay, bool nesterov,
               bool first_step, bool maximize) {
  check_f32_flat(p, "param");
  check_f32_flat(g, "grad");
  if (buf.has_value()) check_f32_flat(*buf, "momentum_buffer");
  launch_fused_sgd<float>(p, g.data_ptr<float>(), buf, lr, momentum,
                          dampening, weight_decay, nesterov, first_step,
                          maximize);
}

void fused_adam(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                torch::Tensor v, double lr, double beta1, double beta2,
                double eps, double weight_decay, bool adamw, double bc1,
                double sqrt_bc2, bool maximize) {
  check_f32_flat(p, "param");
  check_f32_flat(g, "grad");
  check_f32_flat(m, "exp_avg");
  check_f32_flat(v, "exp_avg_sq");
  launch_fused_adam<float>(p, g.data_ptr<float>(), m, v, lr, beta1, beta2,
                           eps, weight_decay, adamw, bc1, sqrt_bc2, maximize);
}

void fused_adagrad(torch::Tensor p, torch::Tensor g, torch::Tensor sum,
                   double clr, double eps, double weight_decay,
                   bool maximize) {
  check_f32_flat(p, "param");
  check_f32_flat(g, "grad");
  check_f32_flat(sum, "sum");
  launch_fused_adagrad<float>(p, g.data_ptr<float>(), sum, clr, eps,
                              weight_decay, maximize);
}

// ---- bf16-gradient ("wire") entry points. The vector paths read 16 B per
// lane from the fp32 streams and 8 B per lane from the bf16 stream at lane
// offsets that are multiples of 4 elements, so every base pointer must be
// 16-byte aligned (shard views of a sharded bucket are: shard lengths are
// multiples of 8 elements). All operands hold the same number of elements.
void check_aligned16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must be 16-byte aligned");
}

void check_wire_f32(const torch::Tensor& t, long n, const char* name) {
  check_f32_flat(t, name);
  check_aligned16(t, name);
  TORCH_CHECK(t.numel() == n, name, " must have ", n, " elements, got ",
              t.numel());
}

const __hip_bfloat16* check_wire_grad(const torch::Tensor& g, long n) {
  TORCH_CHECK(g.is_cuda(), "grad must be on GPU");
  TORCH_CHECK(g.is_contiguous(), "grad must be contiguous");
  TORCH_CHECK(g.scalar_type() == torch::kBFloat16, "grad must be bf16");
  check_aligned16(g, "grad");
  TORCH_CHECK(g.numel() == n, "grad must have ", n, " elements, got ",
              g.numel());
  return reinterpret_cast<const __hip_bfloat16*>(g.data_ptr());
}

void fused_sgd_wire(torch::Tensor p, torch::Tensor g,
                    c10::optional<torch::Tensor> buf, double lr,
                    double momentum, double dampening, double weight_decay,
                    bool nesterov, bool first_step, bool maximize) {
  long n = p.numel();
  check_wire_f32(p, n, "param");
  const __hip_bfloat16* gp = check_wire_grad(g, n);
  if (buf.has_value()) check_wire_f32(*buf, n, "momentum_buffer");
  launch_fused_sgd<__hip_bfloat16>(p, gp, buf, lr, momentum, dampening,
                                   weight_decay, nesterov, first_step,
                                   maximize);
}

void fused_adam_wire(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                     torch::Tensor v, double lr, double beta1, double beta2,
                     double eps, double weight_decay, bool adamw, double bc1,
                     double sqrt_bc2, bool maximize) {
  long n = p.numel();
  check_wire_f32(p, n, "param");
  const __hip_bfloat16* gp = check_wire_grad(g, n);
  check_wire_f32(m, n, "exp_avg");
  check_wire_f32(v, n, "exp_avg_sq");
  launch_fused_adam<__hip_bfloat16>(p, gp, m, v, lr, beta1, beta2, eps,
                                    weight_decay, adamw, bc1, sqrt_bc2,
                                    maximize);
}

void fused_adagrad_wire(torch::Tensor p, torch::Tensor g, torch::Tensor sum,
                        double clr, double eps, double weight_decay,
                        bool maximize) {
  long n = p.numel();
  check_wire_f32(p, n, "param");
  const __hip_bfloat16* gp = check_wire_grad(g, n);
  check_wire_f32(sum, n, "sum");
  launch_fused_adagrad<__hip_bfloat16>(p, gp, sum, clr, eps, weight_decay,
                                       maximize);
}

void fused_rmsprop(torch::Tensor p, torch::Tensor g, torch::Tensor sq,
                   c10::optional<torch::Tensor> ga,
                   c10::optional<torch::Tensor> buf, double lr, double alpha,
                   double eps, double weight_decay, double momentum,
                   bool maximize) {
  check_f32_flat(p, "param");
  check_f32_flat(g, "grad");
  check_f32_flat(sq, "square_avg");
  long n = p.numel();
  float* gap = (ga.has_value() && ga->defined()) ? ga->data_ptr<float>()
                                                 : nullptr;
  float* bufp = (buf.has_value() && buf->defined()) ? buf->data_ptr<float>()
                                                    : nullptr;
  hipLaunchKernelGGL(fused_rmsprop_kernel, dim3(grid_for(n, 1)),
                     dim3(BLOCK_THREADS), 0, cur_stream(),
                     p.data_ptr<float>(), g.data_ptr<float>(),
                     sq.data_ptr<float>(), gap, bufp, n, (float)lr,
                     (float)alpha, (float)(1.0 - alpha), (float)eps,
                     (float)weight_decay, (float)momentum, maximize);
}

void scale_cast_bf16(torch::Tensor in, torch::Tensor out, double scale) {
  check_f32_flat(in, "in");
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16 && out.is_contiguous());
  long n = in.numel();
  hipLaunchKernelGGL(scale_cast_bf16_kernel, dim3(grid_for(n)),
                     dim3(BLOCK_THREADS), 0, cur_stream(),
                     in.data_ptr<float>(),
                     reinterpret_cast<__hip_bfloat16*>(out.data_ptr()), n,
                     (float)scale);
}

void cast_back_f32(torch::Tensor in, torch::Tensor out) {
  TORCH_CHECK(in.scalar_type() == torch::kBFloat16 && in.is_contiguous());
  check_f32_flat(out, "out");
  long n = in.numel();
  hipLaunchKernelGGL(cast_back_f32_kernel, dim3(grid_for(n)),
                     dim3(BLOCK_THREADS), 0, cur_stream(),
                     reinterpret_cast<const __hip_bfloat16*>(in.data_ptr()),
                     out.data_ptr<float>(), n);
}

void ef_compress(torch::Tensor flat, torch::Tensor err, torch::Tensor wire,
                 double scale) {
  check_f32_flat(flat, "flat");
  check_f32_flat(err, "err");
  TORCH_CHECK(wire.scalar_type() == torch::kBFloat16);
  long n = flat.numel();
  hipLaunchKernelGGL(ef_compress_kernel, dim3(grid_for(n, 1)),
                     dim3(BLOCK_THREADS), 0, cur_stream(),
                     flat.data_ptr<float>(), err.data_ptr<float>(),
                     reinterpret_cast<__hip_bfloat16*>(wire.data_ptr()), n,
                     (float)scale);
}

std::tuple<torch::Tensor, torch::Tensor> segment_coalesce(
    torch::Tensor indices, torch::Tensor values) {
  TORCH_CHECK(indices.is_cuda() && values.is_cuda());
  TORCH_CHECK(indices.scalar_type() == torch::kInt64);
  auto vals = values.contiguous().to(torch::kFloat32);
  auto [uniq, inverse] = at::_unique(indices, /*sorted=*/true,
                                     /*return_inverse=*/true);
  long dim = values.numel() / std::max<long>(values.size(0), 1);
  auto out_sizes = values.sizes().vec();
  out_sizes[0] = uniq.size(0);
  auto out = torch::zeros(out_sizes, vals.options());
  long nnz = indices.numel();
  if (nnz > 0) {
    hipLaunchKernelGGL(scatter_add_rows_kernel,
                       dim3(grid_for(nnz * dim, 1)), dim3(BLOCK_THREADS), 0,
                       cur_stream(), out.data_ptr<float>(),
                       inverse.contiguous().data_ptr<int64_t>(),
                       vals.data_ptr<float>(), nnz, dim);
  }
  return {uniq, out.to(values.scalar_type())};
}

void scatter_add_rows(torch::Tensor out, torch::Tensor idx,
                      torch::Tensor vals) {
  check_f32_flat(out, "out");
  TORCH_CHECK(idx.scalar_type() == torch::kInt64);
  long nnz = idx.numel();
  long dim = vals.numel() / std::max<long>(nnz, 1);
  if (nnz == 0) return;
  hipLaunchKernelGGL(scatter_add_rows_kernel, dim3(grid_for(nnz * dim, 1)),
                     dim3(BLOCK_THREADS), 0, cur_stream(),
                     out.data_ptr<float>(), idx.contiguous().data_ptr<int64_t>(),
                     vals.contiguous().data_ptr<float>(), nnz, dim);
}

torch::Tensor gather_rows(torch::Tensor src, torch::Tensor idx) {
  check_f32_flat(src, "src");
  TORCH_CHECK(idx.scalar_type() == torch::kInt64);
  long nrows = idx.numel();
  long dim = src.size(1);
  auto out = torch::empty({nrows, dim}, src.options());
  if (nrows > 0) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for(nrows * dim, 1)),
                       dim3(BLOCK_THREADS), 0, cur_stream(),
                       src.data_ptr<float>(), idx.contiguous().data_ptr<int64_t>(),
                       out.data_ptr<float>(), nrows, dim);
  }
  return out;
}

// Row-wise optimizer apply for unique rows (see multi_tensor.hip). opt:
// 0 = SGD, 1 = Adagrad (lr is the host-decayed clr), 2 = Adam/SparseAdam.
template <int OPT>
static void launch_sparse_apply(bool vec4, dim3 grid, float* p,
                                const int64_t* rows, const float* g,
                                float* s1, float* s2, float* out, long n,
                                long R, long D, long row_base, int log2_group,
                                SparseHyper h) {
  if (vec4) {
    hipLaunchKernelGGL((sparse_apply_rows_kernel<OPT, 4>), grid,
                       dim3(BLOCK_THREADS), 0, cur_stream(), p, rows, g, s1,
                       s2, out, n, R, D, row_base, log2_group, h);
  } else {
    hipLaunchKernelGGL((sparse_apply_rows_kernel<OPT, 1>), grid,
                       dim3(BLOCK_THREADS), 0, cur_stream(), p, rows, g, s1,
                       s2, out, n, R, D, row_base, log2_group, h);
  }
}

static bool aligned16(const void* ptr) {
  return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0;
}

void sparse_apply_rows(int64_t opt, torch::Tensor param, torch::Tensor rows,
                       torch::Tensor row_grads,
                       c10::optional<torch::Tensor> state1,
                       c10::optional<torch::Tensor> state2,
                       c10::optional<torch::Tensor> new_rows, int64_t row_base,
                       double lr, double beta1, double beta2, double eps,
                       double bc1, double sqrt_bc2) {
  TORCH_CHECK(opt >= SPARSE_SGD && opt <= SPARSE_ADAM, "unknown optimizer id");
  check_f32_flat(param, "param");
  check_f32_flat(row_grads, "row_grads");
  TORCH_CHECK(rows.is_cuda() && rows.is_contiguous() && rows.dim() == 1 &&
              rows.scalar_type() == torch::kInt64,
              "rows must be a contiguous 1-D int64 GPU tensor");
  TORCH_CHECK(param.dim() >= 1, "param must have a row dimension");
  TORCH_CHECK(row_base >= 0, "row_base must be non-negative");
  long n = rows.numel();
  long R = param.size(0);
  long D = R > 0 ? param.numel() / R : 0;
  TORCH_CHECK(R == 0 || row_grads.numel() == n * D,
              "row_grads must be [n, D]");
  bool has1 = state1.has_value() && state1->defined();
  bool has2 = state2.has_value() && state2->defined();
  TORCH_CHECK(has1 == (opt != SPARSE_SGD) && has2 == (opt == SPARSE_ADAM),
              "state tensors do not match the optimizer");
  float* s1 = nullptr;
  float* s2 = nullptr;
  if (has1) {
    check_f32_flat(*state1, "state1");
    TORCH_CHECK(state1->numel() == param.numel(), "state1 must be [R, D]");
    s1 = state1->data_ptr<float>();
  }
  if (has2) {
    check_f32_flat(*state2, "state2");
    TORCH_CHECK(state2->numel() == param.numel(), "state2 must be [R, D]");
    s2 = state2->data_ptr<float>();
  }
  float* out = nullptr;
  if (new_rows.has_value() && new_rows->defined()) {
    check_f32_flat(*new_rows, "new_rows");
    TORCH_CHECK(new_rows->numel() == row_grads.numel(),
                "new_rows must be [n, D]");
    out = new_rows->data_ptr<float>();
  }
  if (n == 0 || R == 0 || D == 0) return;  // nothing to launch
  float* p = param.data_ptr<float>();
  const float* g = row_grads.data_ptr<float>();
  // float4 path needs every row start 16-byte aligned: D % 4 == 0 and
  // aligned bases (a narrow(0, ..) shard view keeps alignment when D % 4 == 0)
  bool vec4 = D % 4 == 0 && aligned16(p) && aligned16(g) &&
              (s1 == nullptr || aligned16(s1)) &&
              (s2 == nullptr || aligned16(s2)) &&
              (out == nullptr || aligned16(out));
  long chunks = vec4 ? D / 4 : D;
  int log2_group = 0;
  while (log2_group < 6 && (1L << log2_group) < chunks) ++log2_group;
  long rows_per_block = BLOCK_THREADS >> log2_group;
  long blocks = (n + rows_per_block - 1) / rows_per_block;
  if (blocks > 65535L * 8) blocks = 65535L * 8;
  dim3 grid((unsigned)blocks);
  SparseHyper h{(float)lr, (float)beta1, (float)beta2, (float)(1.0 - beta1),
                (float)(1.0 - beta2), (float)eps, (float)bc1, (float)sqrt_bc2};
  const int64_t* rp = rows.data_ptr<int64_t>();
  if (opt == SPARSE_SGD) {
    launch_sparse_apply<SPARSE_SGD>(vec4, grid, p, rp, g, s1, s2, out, n, R,
                                    D, row_base, log2_group, h);
  } else if (opt == SPARSE_ADAGRAD) {
    launch_sparse_apply<SPARSE_ADAGRAD>(vec4, grid, p, rp, g, s1, s2, out, n,
                                        R, D, row_base, log2_group, h);
  } else {
    launch_sparse_apply<SPARSE_ADAM>(vec4, grid, p, rp, g, s1, s2, out, n, R,
                                     D, row_base, log2_group, h);
  }
}

// ------------------------------------------------------------- PowerSGD
torch::Tensor psgd_mq(torch::Tensor M2d, torch::Tensor Qp) {
  long n = M2d.size(0), s = M2d.size(1);
  TORCH_CHECK(n % 64 == 0 && s % 64 == 0, "psgd_mq needs 64-multiples");
  TORCH_CHECK(Qp.size(0) == s && Qp.size(1) == PSGD_R);
  auto C = torch::zeros({n, (long)PSGD_R},
                        M2d.options().dtype(torch::kFloat32));
  long gridx = n / 64;
  long chunks = s / PSGD_BK;
  long splitk = std::min(std::max<long>((512 + gridx - 1) / gridx, 1), chunks);
  hipLaunchKernelGGL(psgd_mq_kernel, dim3(gridx, splitk), dim3(256), 0,
                     cur_stream(), M2d.data_ptr<float>(),
                     Qp.contiguous().data_ptr<float>(), C.data_ptr<float>(),
                     n, s);
  return C;
}

torch::Tensor psgd_mtp(torch::Tensor M2d, torch::Tensor Pp) {
  long n = M2d.size(0), s = M2d.size(1);
  TORCH_CHECK(n % 64 == 0 && s % 64 == 0, "psgd_mtp needs 64-multiples");
  TORCH_CHECK(Pp.size(0) == n && Pp.size(1) == PSGD_R);
  auto C = torch::zeros({s, (long)PSGD_R},
                        M2d.options().dtype(torch::kFloat32));
  long gridx = s / 64;
  long chunks = n / PSGD_BK;
  long splitk = std::min(std::max<long>((512 + gridx - 1) / gridx, 1), chunks);
  hipLaunchKernelGGL(psgd_mtp_kernel, dim3(gridx, splitk), dim3(256), 0,
                     cur_stream(), M2d.data_ptr<float>(),
                     Pp.contiguous().data_ptr<float>(), C.data_ptr<float>(),
                     n, s);
  return C;
}

void psgd_decompress_ef(torch::Tensor flat, torch::Tensor err,
                        torch::Tensor m_local, torch::Tensor Pp,
                        torch::Tensor Qp, double scale) {
  long numel = flat.numel();
  long s = m_local.size(1);
  hipLaunchKernelGGL(psgd_decompress_ef_kernel, dim3(grid_for(numel, 1)),
                     dim3(BLOCK_THREADS), 0, cur_stream(),
                     flat.data_ptr<float>(), err.data_ptr<float>(),
                     m_local.data_ptr<float>(), Pp.data_ptr<float>(),
                     Qp.data_ptr<float>(), numel, s, (float)scale);
}

// Q/K/V may be views of a fused qkv projection: last dim must be
// contiguous, other dims carried as element strides into the kernels.
static void attn_check_strided(const torch::Tensor& t, long D,
                               const char* name) {
  TORCH_CHECK(t.dim() == 4 && t.size(3) == D && t.stride(3) == 1,
              name, ": expected [B,H,S,D] with contiguous head dim");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16);
}

static const float* attn_mask_ptr(const c10::optional<torch::Tensor>& mask,
                                  long B, long S) {
  if (!mask.has_value() || !mask->defined()) return nullptr;
  TORCH_CHECK(mask->scalar_type() == torch::kFloat32 && mask->is_contiguous(),
              "attention mask must be contiguous fp32");
  TORCH_CHECK(mask->numel() == B * S,
              "attention mask must be an additive [B,1,1,S] key mask");
  return mask->data_ptr<float>();
}

torch::Tensor attn_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                       double scale,
                       c10::optional<torch::Tensor> mask = c10::nullopt,
                       double p_drop = 0.0, int64_t seed = 0) {
  long D = q.size(3);
  TORCH_CHECK(q.dim() == 4 && (D == 64 || D == 128),
              "attn_fwd expects [B,H,S,64|128]");
  attn_check_strided(q, D, "q");
  attn_check_strided(k, D, "k");
  attn_check_strided(v, D, "v");
  long B = q.size(0), H = q.size(1), S = q.size(2);
  TORCH_CHECK(S % 32 == 0 && S >= 32, "S must be a multiple of 32");
  TORCH_CHECK(k.sizes() == q.sizes() && v.sizes() == q.sizes());
  auto o = torch::empty({B, H, S, D}, q.options());
  // RB=2 (128-row blocks) halves K/V re-read traffic for long sequences;
  // RB=1 keeps more blocks in flight for short ones. 1-D grid with bh as
  // the fast dimension = XCD-locality swizzle (see kernel comment).
  long nbh = B * H;
  auto launch = [&](auto kern, long rows) {
    long nqb = (S + rows - 1) / rows;
    hipLaunchKernelGGL(kern, dim3(nqb * nbh), dim3(256), 0, cur_stream(),
                       reinterpret_cast<__hip_bfloat16*>(q.data_ptr()),
                       reinterpret_cast<__hip_bfloat16*>(k.data_ptr()),
                       reinterpret_cast<__hip_bfloat16*>(v.data_ptr()),
                       reinterpret_cast<__hip_bfloat16*>(o.data_ptr()),
                       attn_mask_ptr(mask, B, S), S, H, nbh,
                       q.stride(0), q.stride(1), q.stride(2),
                       k.stride(0), k.stride(1), k.stride(2),
                       v.stride(0), v.stride(1), v.stride(2),
                       (float)scale, (float)p_drop,
                       (unsigned int)(uint64_t)seed);
  };
  // RB=3 (192-row blocks) for S>=512 was MEASURED SLOWER (0.034 -> 0.048
  // ms at S=512): occupancy 3 -> 2 waves/SIMD plus partial-tile waste
  // outweigh the traffic saving. RB=2 is the sweet spot.
  if (q.size(3) == 64) {
    if (S >= 256) launch(attn_fwd_kernel<2, 64>, 128);
    else launch(attn_fwd_kernel<1, 64>, 64);
  } else {
    if (S >= 256) launch(attn_fwd_kernel<2, 128>, 128);
    else launch(attn_fwd_kernel<1, 128>, 64);
  }
  return o;
}

torch::Tensor attn_dropmask(long B, long H, long S, double p_drop,
                            int64_t seed, torch::Device dev) {
  auto out = torch::empty({B, H, S, S},
                          torch::dtype(torch::kUInt8).device(dev));
  hipLaunchKernelGGL(attn_dropmask_kernel, dim3(S, B * H), dim3(256), 0,
                     cur_stream(), out.data_ptr<unsigned char>(), S,
                     (float)p_drop, (unsigned int)(uint64_t)seed);
  return out;
}

std::vector<torch::Tensor> attn_bwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, torch::Tensor o,
                                    torch::Tensor dout, double scale,
                                    c10::optional<torch::Tensor> mask
                                        = c10::nullopt,
                                    double p_drop = 0.0, int64_t seed = 0) {
  long D = q.size(3);
  TORCH_CHECK(q.dim() == 4 && (D == 64 || D == 128));
  attn_check_strided(q, D, "q");
  attn_check_strided(k, D, "k");
  attn_check_strided(v, D, "v");
  TORCH_CHECK(o.is_contiguous() && dout.is_contiguous());
  long B = q.size(0), H = q.size(1), S = q.size(2);
  TORCH_CHECK(S % 32 == 0 && S >= 32);
  auto dq = torch::empty({B, H, S, D}, q.options());
  auto dk = torch::empty({B, H, S, D}, q.options());
  auto dv = torch::empty({B, H, S, D}, q.options());
  auto fopt = q.options().dtype(torch::kFloat32);
  auto Mbuf = torch::empty({B * H * S}, fopt);
  auto Lbuf = torch::empty({B * H * S}, fopt);
  auto Dbuf = torch::empty({B * H * S}, fopt);
  const float* mp = attn_mask_ptr(mask, B, S);
  unsigned int sd = (unsigned int)(uint64_t)seed;
  // 1-D grids, (b,h) fast for XCD L2 locality (see attention.hip)
  long nbh = B * H;
  dim3 grid(((S + 63) / 64) * nbh);
  auto st = cur_stream();
#define BF16P(t) reinterpret_cast<__hip_bfloat16*>((t).data_ptr())
  if (q.size(3) == 64) {
    hipLaunchKernelGGL(attn_bwd_q_kernel<64>, grid, dim3(256), 0, st,
                       BF16P(q), BF16P(k), BF16P(v), BF16P(o), BF16P(dout),
                       BF16P(dq), Mbuf.data_ptr<float>(),
                       Lbuf.data_ptr<float>(), Dbuf.data_ptr<float>(), mp,
                       S, H, nbh, q.stride(0), q.stride(1), q.stride(2),
                       k.stride(0), k.stride(1), k.stride(2), v.stride(0),
                       v.stride(1), v.stride(2), (float)scale,
                       (float)p_drop, sd);
    hipLaunchKernelGGL(attn_bwd_kv_kernel<64>, grid, dim3(256), 0, st,
                       BF16P(q), BF16P(k), BF16P(v), BF16P(dout), BF16P(dk),
                       BF16P(dv), Mbuf.data_ptr<float>(),
                       Lbuf.data_ptr<float>(), Dbuf.data_ptr<float>(), mp,
                       S, H, nbh, q.stride(0), q.stride(1), q.stride(2),
                       k.stride(0), k.stride(1), k.stride(2), v.stride(0),
                       v.stride(1), v.stride(2), (float)scale,
                       (float)p_drop, sd);
  } else {
    hipLaunchKernelGGL(attn_bwd_q_kernel<128>, grid, dim3(256), 0, st,
                       BF16P(q), BF16P(k), BF16P(v), BF16P(o), BF16P(dout),
                       BF16P(dq), Mbuf.data_ptr<float>(),
                       Lbuf.data_ptr<float>(), Dbuf.data_ptr<float>(), mp,
                       S, H, nbh, q.stride(0), q.stride(1), q.stride(2),
                       k.stride(0), k.stride(1), k.stride(2), v.stride(0),
                       v.stride(1), v.stride(2), (float)scale,
                       (float)p_drop, sd);
    hipLaunchKernelGGL(attn_bwd_kv_kernel<128>, grid, dim3(256), 0, st,
                       BF16P(q), BF16P(k), BF16P(v), BF16P(dout), BF16P(dk),
                       BF16P(dv), Mbuf.data_ptr<float>(),
                       Lbuf.data_ptr<float>(), Dbuf.data_ptr<float>(), mp,
                       S, H, nbh, q.stride(0), q.stride(1), q.stride(2),
                       k.stride(0), k.stride(1), k.stride(2), v.stride(0),
                       v.stride(1), v.stride(2), (float)scale,
                       (float)p_drop, sd);
  }
#undef BF16P
  return {dq, dk, dv};
}

std::vector<torch::Tensor> ln_fwd(torch::Tensor x,
                                  c10::optional<torch::Tensor> res,
                                  torch::Tensor gamma, torch::Tensor beta,
                                  double eps) {
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 && x.is_contiguous());
  long H = x.size(-1);
  long N = x.numel() / H;
  TORCH_CHECK(H <= 4096 && H % 2 == 0,
              "ln_fwd supports even H <= 4096");
  TORCH_CHECK(gamma.scalar_type() == torch::kFloat32 && gamma.is_contiguous());
  auto y = torch::empty_like(x);
  bool has_res = res.has_value() && res->defined();
  torch::Tensor u = has_res ? torch::empty_like(x) : x;
  auto fopt = x.options().dtype(torch::kFloat32);
  auto mean = torch::empty({N}, fopt);
  auto rstd = torch::empty({N}, fopt);
  const __hip_bfloat16* rp = has_res
      ? reinterpret_cast<__hip_bfloat16*>(res->data_ptr()) : nullptr;
  __hip_bfloat16* up = has_res
      ? reinterpret_cast<__hip_bfloat16*>(u.data_ptr()) : nullptr;
  hipLaunchKernelGGL(ln_fwd_kernel, dim3(N), dim3(256), 0, cur_stream(),
                     reinterpret_cast<__hip_bfloat16*>(x.data_ptr()), rp,
                     gamma.data_ptr<float>(), beta.data_ptr<float>(),
                     reinterpret_cast<__hip_bfloat16*>(y.data_ptr()), up,
                     mean.data_ptr<float>(), rstd.data_ptr<float>(), N,
                     (int)H, (float)eps);
  return {y, u, mean, rstd};
}

std::vector<torch::Tensor> ln_bwd(torch::Tensor dy, torch::Tensor u,
                                  torch::Tensor gamma, torch::Tensor mean,
                                  torch::Tensor rstd) {
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16 && dy.is_contiguous());
  long H = dy.size(-1);
  long N = dy.numel() / H;
  auto dx = torch::empty_like(dy);
  hipLaunchKernelGGL(ln_bwd_dx_kernel, dim3(N), dim3(256), 0, cur_stream(),
                     reinterpret_cast<__hip_bfloat16*>(dy.data_ptr()),
                     reinterpret_cast<__hip_bfloat16*>(u.data_ptr()),
                     gamma.data_ptr<float>(), mean.data_ptr<float>(),
                     rstd.data_ptr<float>(),
                     reinterpret_cast<__hip_bfloat16*>(dx.data_ptr()), N,
                     (int)H);
  // chunked dgamma/dbeta partials, reduced on the torch side
  long rows_per_chunk = 256;
  long nchunks = (N + rows_per_chunk - 1) / rows_per_chunk;
  auto partials = torch::empty({nchunks, 2, H},
                               dy.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL(ln_bwd_gb_kernel, dim3((H + 63) / 64, nchunks),
                     dim3(256), 0, cur_stream(),
                     reinterpret_cast<__hip_bfloat16*>(dy.data_ptr()),
                     reinterpret_cast<__hip_bfloat16*>(u.data_ptr()),
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),
                     partials.data_ptr<float>(), N, (int)H, rows_per_chunk);
  auto gb = partials.sum(0);
  return {dx, gb[0], gb[1]};
}

torch::Tensor col_sum(torch::Tensor x) {
  TORCH_CHECK(x.dim() == 2 && x.scalar_type() == torch::kBFloat16 &&
              x.is_contiguous());
  long N = x.size(0), H = x.size(1);
  // chunk rows so the grid fills the 8 XCDs even for narrow H
  long rows_per_chunk = 512;
  long nchunks = (N + rows_per_chunk - 1) / rows_per_chunk;
  if (nchunks > 256) { nchunks = 256;
    rows_per_chunk = (N + nchunks - 1) / nchunks; }
  auto partials = torch::empty({nchunks, H},
                               x.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL(col_sum_kernel, dim3((H + 63) / 64, nchunks),
                     dim3(256), 0, cur_stream(),
                     reinterpret_cast<__hip_bfloat16*>(x.data_ptr()),
                     partials.data_ptr<float>(), N, H, rows_per_chunk);
  return partials.sum(0);
}

std::vector<torch::Tensor> ce_fwd(torch::Tensor logits,
                                  torch::Tensor targets) {
  TORCH_CHECK(logits.dim() == 2 && logits.scalar_type() == torch::kBFloat16
              && logits.is_contiguous());
  TORCH_CHECK(targets.scalar_type() == torch::kLong);
  long N = logits.size(0), H = logits.size(1);
  auto fopt = logits.options().dtype(torch::kFloat32);
  auto loss_rows = torch::empty({N}, fopt);
  auto m = torch::empty({N}, fopt);
  auto l2s = torch::empty({N}, fopt);
  hipLaunchKernelGGL(ce_fwd_kernel, dim3(N), dim3(256), 0, cur_stream(),
                     reinterpret_cast<__hip_bfloat16*>(logits.data_ptr()),
                     targets.data_ptr<long>(), loss_rows.data_ptr<float>(),
                     m.data_ptr<float>(), l2s.data_ptr<float>(), N, H);
  return {loss_rows, m, l2s};
}

torch::Tensor ce_bwd(torch::Tensor logits, torch::Tensor targets,
                     torch::Tensor m, torch::Tensor l2s,
                     torch::Tensor dloss_rows) {
  long N = logits.size(0), H = logits.size(1);
  auto dlogits = torch::empty_like(logits);
  hipLaunchKernelGGL(ce_bwd_kernel, dim3(N), dim3(256), 0, cur_stream(),
                     reinterpret_cast<__hip_bfloat16*>(logits.data_ptr()),
                     targets.data_ptr<long>(), m.data_ptr<float>(),
                     l2s.data_ptr<float>(),
                     dloss_rows.contiguous().data_ptr<float>(),
                     reinterpret_cast<__hip_bfloat16*>(dlogits.data_ptr()),
                     N, H);
  return dlogits;
}

torch::Tensor mfma_probe(torch::Tensor A, torch::Tensor B, long cand) {
  TORCH_CHECK(A.scalar_type() == torch::kBFloat16 && A.numel() == 16 * 32);
  TORCH_CHECK(B.scalar_type() == torch::kBFloat16 && B.numel() == 32 * 16);
  auto D = torch::zeros({16, 16}, A.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, cur_stream(),
                     reinterpret_cast<__hip_bfloat16*>(A.data_ptr()),
                     reinterpret_cast<__hip_bfloat16*>(B.data_ptr()),
                     D.data_ptr<float>(), (int)cand);
  return D;
}

void psgd_add_err_pad(torch::Tensor flat, torch::Tensor err,
                      torch::Tensor out) {
  long numel = flat.numel();
  long total = out.numel();
  hipLaunchKernelGGL(psgd_add_err_pad_kernel, dim3(grid_for(total, 1)),
                     dim3(BLOCK_THREADS), 0, cur_stream(),
                     flat.data_ptr<float>(), err.data_ptr<float>(),
                     out.data_ptr<float>(), numel, total);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("fused_sgd", &fused_sgd, "fused flat SGD update (gfx950)");
  m.def("fused_adam", &fused_adam, "fused flat Adam/AdamW update (gfx950)");
  m.def("fused_adagrad", &fused_adagrad,
        "fused flat Adagrad update (gfx950)");
  m.def("fused_sgd_wire", &fused_sgd_wire,
        "fused flat SGD update, bf16 wire gradient (gfx950)");
  m.def("fused_adam_wire", &fused_adam_wire,
        "fused flat Adam/AdamW update, bf16 wire gradient (gfx950)");
  m.def("fused_adagrad_wire", &fused_adagrad_wire,
        "fused flat Adagrad update, bf16 wire gradient (gfx950)");
  m.def("fused_rmsprop", &fused_rmsprop,
        "fused flat RMSprop update (gfx950, centered/momentum variants)");
  m.def("scale_cast_bf16", &scale_cast_bf16, "scale+cast fp32->bf16");
  m.def("cast_back_f32", &cast_back_f32, "cast bf16->fp32");
  m.def("ef_compress", &ef_compress, "fused error-feedback bf16 compress");
  m.def("segment_coalesce", &segment_coalesce,
        "dedup-sum row-sparse gradient");
  m.def("scatter_add_rows", &scatter_add_rows, "rowwise scatter-add");
  m.def("gather_rows", &gather_rows, "rowwise gather");
  m.def("sparse_apply_rows", &sparse_apply_rows,
        "fused row-wise SGD/Adagrad/Adam update of unique rows (gfx950)");
  m.def("bn_fwd_train", &bn_fwd_train,
        "fused NHWC batchnorm fwd (+add+relu), returns y/save_mean/save_rstd");
  m.def("bn_bwd", &bn_bwd,
        "fused NHWC batchnorm bwd (+relu-mask+dres), returns "
        "dx/dweight/dbias[/dres]");
  m.def("bn_fwd_train_mask", &bn_fwd_train_mask,
        "bn_fwd_train with relu that also returns the bit-packed ReLU mask "
        "[M, C/8] uint8");
  m.def("bn_bwd_mask", &bn_bwd_mask,
        "bn_bwd that takes the packed mask of bn_fwd_train_mask in place of "
        "y");
  m.def("bn_bwd_mask_join", &bn_bwd_mask_join,
        "bn_bwd_mask for dy = dy_a + dy_b, the add done in the reduce: (x, "
        "dy_a, dy_b, mask, save_mean, save_rstd, weight, ws) -> (dx, "
        "dweight, dbias, dz); dz is the masked sum, the split path's dres");
  m.def("bn_bwd_mask_join", &bn_bwd_mask_join_bn,
        "the same for the tail relu(bn(z) + bn_d(zd)), both branches in one "
        "reduce and one apply: (z, dy_a, dy_b, mask, save_mean, save_rstd, "
        "weight, ws, zd, save_mean_d, save_rstd_d, weight_d, ws_d) -> (dx, "
        "dweight, dbias, dz, dx_d, dweight_d, dbias_d), what the one-BN call "
        "on z and bn_bwd(zd, dz) return");
  m.def("bn_fwd_train_pool", &bn_fwd_train_pool,
        "bn + relu + 3x3/stride 2/pad 1 max-pool: (x, weight, bias, "
        "running_mean, running_var, eps, momentum, ws) -> (pooled y, "
        "save_mean, save_rstd, argmax words)");
  m.def("bn_bwd_pool", &bn_bwd_pool,
        "backward of bn_fwd_train_pool: (x, dy_pooled, argmax, save_mean, "
        "save_rstd, weight, ws) -> (dx, dweight, dbias)");
  m.def("bn_fwd_train_add_bn", &bn_fwd_train_add_bn,
        "relu(bn(z) + bn_d(zd)): (z, zd, then weight, bias, running_mean, "
        "running_var, eps, momentum, ws of each BN) -> (y, mask, save_mean, "
        "save_rstd, save_mean_d, save_rstd_d)");
  // rows in flight per thread in the BN reduce / finalize loops
  m.attr("BN_RED_U") = BN_RED_U;
  m.attr("BN_FIN_U") = BN_FIN_U;
  m.attr("BN_JOIN_U") = BN_JOIN_U;
  m.attr("BN_JOIN2_U") = BN_JOIN2_U;
  // and in the streaming apply kernels (tests mirror bn_apply_gm with them)
  m.attr("BN_APPLY_FWD_U") = BN_APPLY_FWD_U;
  m.attr("BN_APPLY_BWD_U") = BN_APPLY_BWD_U;
  m.attr("BN_APPLY2_U") = BN_APPLY2_U;
  m.def("psgd_mq", &psgd_mq, "PowerSGD P = M @ Q (MFMA f32 16x16x4)");
  m.def("psgd_mtp", &psgd_mtp, "PowerSGD Qn = M^T @ P (MFMA f32 16x16x4)");
  m.def("psgd_decompress_ef", &psgd_decompress_ef,
        "fused hat = P Q^T * scale; err = M - hat; flat = hat");
  m.def("psgd_add_err_pad", &psgd_add_err_pad,
        "padded M = flat + err (zero tail)");
  m.def("mfma_probe", &mfma_probe,
        "diagnostic: v_mfma_f32_16x16x32_bf16 A/B layout probe");
  m.def("ce_fwd", &ce_fwd,
        "fused online-softmax cross-entropy fwd -> loss_rows, m, l2s");
  m.def("ce_bwd", &ce_bwd, "fused cross-entropy bwd -> dlogits (bf16)");
  m.def("col_sum", &col_sum, "bf16 [N,H] column sum -> fp32 [H]");
  m.def("ln_fwd", &ln_fwd,
        "fused bf16 LayerNorm(+residual) forward -> y, u, mean, rstd");
  m.def("ln_bwd", &ln_bwd, "fused bf16 LayerNorm backward -> dx, dgamma, "
        "dbeta");
  m.def("attn_dropmask", &attn_dropmask,
        "materialize the hash dropout keep-mask (testing)");
  m.def("attn_fwd", &attn_fwd,
        "fused MFMA attention forward (bf16, D=64; optional additive key "
        "mask + hash dropout) — 4-wave LDS-tiled",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("scale"),
        py::arg("mask") = py::none(), py::arg("p_drop") = 0.0,
        py::arg("seed") = 0);
  m.def("attn_bwd", &attn_bwd,
        "fused MFMA attention backward (GPU-validated) -> dq, dk, dv",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
        py::arg("dout"), py::arg("scale"), py::arg("mask") = py::none(),
        py::arg("p_drop") = 0.0, py::arg("seed") = 0);
}
