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
#include "attention_split.hip"
#include "attention_bwd.hip"
#include "ln_ops.hip"
#include "ce_ops.hip"
#include "lstm_ops.hip"
#include "ssm_ops.hip"
#include "lce_ops.hip"
#include "ncf_ops.hip"
#include "sparse_ops.hip"

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

// Sort-free deterministic coalesce (see sparse_ops.hip). workspace is the
// caller's persistent int32 buffer for this table height, bitmap part all
// zero on entry and again on exit. Returns (uniq[n], out[n, D], count[1]),
// padded; nothing here reads the device.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> coalesce_rows_ranked(
    torch::Tensor ids, torch::Tensor vals, int64_t num_rows,
    torch::Tensor workspace, double scale) {
  TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == torch::kInt64 &&
              ids.dim() == 1 && ids.is_contiguous(),
              "ids must be a contiguous 1-D int64 GPU tensor");
  check_f32_flat(vals, "vals");
  TORCH_CHECK(num_rows >= 1 && num_rows < (1LL << 31),
              "num_rows must be in [1, 2^31), got ", num_rows);
  long n = ids.numel();
  TORCH_CHECK(n < (1LL << 31), "at most 2^31 - 1 input rows");
  TORCH_CHECK(vals.dim() >= 1 && vals.size(0) == n,
              "vals must have one row per id");
  long R = num_rows;
  long W = (R + 31) / 32;
  long nblk = (W + BLOCK_THREADS - 1) / BLOCK_THREADS;
  TORCH_CHECK(workspace.is_cuda() && workspace.is_contiguous() &&
              workspace.scalar_type() == torch::kInt32 &&
              workspace.numel() >= 2 * W + nblk &&
              workspace.device() == ids.device() &&
              vals.device() == ids.device(),
              "workspace must be an int32 tensor of 2*ceil(R/32) + "
              "ceil(ceil(R/32)/256) words on the ids' device");
  auto iopt = ids.options();
  auto uniq = torch::empty({n}, iopt);
  auto out = torch::empty_like(vals);
  if (n == 0)
    return {uniq, out, torch::zeros({1}, iopt.dtype(torch::kInt32))};
  long D = vals.numel() / n;
  TORCH_CHECK(D > 0, "vals rows must not be empty");
  auto count = torch::empty({1}, iopt.dtype(torch::kInt32));
  auto scratch = torch::empty({4 * n + 1}, iopt.dtype(torch::kInt32));
  int* ws = workspace.data_ptr<int>();
  unsigned int* bitmap = reinterpret_cast<unsigned int*>(ws);
  int* prefix = ws + W;
  int* blocksum = ws + 2 * W;
  int* sc = scratch.data_ptr<int>();
  int* slot = sc;
  int* cnt = sc + n;
  int* start = sc + 2 * n;
  int* perm = sc + 3 * n;
  int* cursor = sc + 4 * n;
  int* cp = count.data_ptr<int>();
  const int64_t* ip = ids.data_ptr<int64_t>();
  const float* vp = vals.data_ptr<float>();
  float* op = out.data_ptr<float>();
  int64_t* up = uniq.data_ptr<int64_t>();
  hipStream_t st = cur_stream();
  dim3 blk(BLOCK_THREADS);
  dim3 grid_n(grid_for(n, 1));
  dim3 grid_w((unsigned)std::min<long>(nblk, 65535L * 8));
  hipLaunchKernelGGL(coalesce_mark_kernel, grid_n, blk, 0, st, ip, bitmap,
                     cnt, cursor, n, R);
  hipLaunchKernelGGL(coalesce_totals_kernel, grid_w, blk, 0, st, bitmap,
                     blocksum, W);
  hipLaunchKernelGGL(coalesce_scan_kernel, dim3(1), blk, 0, st, blocksum, cp,
                     nblk);
  hipLaunchKernelGGL(coalesce_emit_kernel, grid_w, blk, 0, st, bitmap,
                     blocksum, prefix, up, W, n);
  hipLaunchKernelGGL(coalesce_count_kernel, grid_n, blk, 0, st, ip, bitmap,
                     prefix, slot, cnt, n, R);
  hipLaunchKernelGGL(coalesce_alloc_kernel, grid_n, blk, 0, st, cnt, start,
                     cursor, cp, n);
  hipLaunchKernelGGL(coalesce_place_kernel, grid_n, blk, 0, st, ip, slot,
                     start, perm, bitmap, n);
  bool vec4 = D % 4 == 0 && aligned16(vp) && aligned16(op);
  long chunks = vec4 ? D / 4 : D;
  int log2_group = 0;
  while (log2_group < 6 && (1L << log2_group) < chunks) ++log2_group;
  long rows_per_block = BLOCK_THREADS >> log2_group;
  long blocks = (n + rows_per_block - 1) / rows_per_block;
  if (blocks > 65535L * 8) blocks = 65535L * 8;
  dim3 grid_s((unsigned)blocks);
  if (vec4) {
    hipLaunchKernelGGL((coalesce_sum_kernel<4>), grid_s, blk, 0, st, vp, slot,
                       cnt, start, perm, cp, op, up, n, D, log2_group,
                       (float)scale);
  } else {
    hipLaunchKernelGGL((coalesce_sum_kernel<1>), grid_s, blk, 0, st, vp, slot,
                       cnt, start, perm, cp, op, up, n, D, log2_group,
                       (float)scale);
  }
  return {uniq, out, count};
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

// Split-KV forward (attention_split.hip): kv_splits workgroups share the keys
// of one (b, h, query block), a second kernel merges their partial softmaxes.
// The count is clamped to ATTN_MAX_SPLITS and to the T = ceil(S / 64) tiles,
// and the effective count ceil(T / ceil(T / n)) leaves no split empty, so
// every workgroup's first tile starts below S. p_drop exists to be refused:
// dropout stays on attn_fwd.
torch::Tensor attn_fwd_split(torch::Tensor q, torch::Tensor k,
                             torch::Tensor v, double scale,
                             c10::optional<torch::Tensor> mask,
                             int64_t kv_splits, double p_drop = 0.0) {
  TORCH_CHECK(p_drop == 0.0, "attn_fwd_split has no dropout; use attn_fwd");
  TORCH_CHECK(kv_splits >= 1, "kv_splits must be >= 1, got ", kv_splits);
  TORCH_CHECK(q.dim() == 4 && (q.size(3) == 64 || q.size(3) == 128),
              "attn_fwd_split expects [B,H,S,64|128]");
  long D = q.size(3);
  attn_check_strided(q, D, "q");
  attn_check_strided(k, D, "k");
  attn_check_strided(v, D, "v");
  long B = q.size(0), H = q.size(1), S = q.size(2);
  TORCH_CHECK(S % 32 == 0 && S >= 32, "S must be a multiple of 32");
  TORCH_CHECK(k.sizes() == q.sizes() && v.sizes() == q.sizes());
  long nbh = B * H;
  long T = (S + 63) / 64;
  long n = std::min<long>(std::min<long>(kv_splits, ATTN_MAX_SPLITS), T);
  long tps = (T + n - 1) / n;
  n = (T + tps - 1) / tps;
  auto o = torch::empty({B, H, S, D}, q.options());
  auto f32 = q.options().dtype(torch::kFloat32);
  auto o_part = torch::empty({n, nbh, S, D}, f32);
  auto ml_part = torch::empty({2, n, nbh, S}, f32);
  float* m_part = ml_part.data_ptr<float>();
  float* l_part = m_part + n * nbh * S;
  auto launch = [&](auto kern, long rows) {
    long nqb = (S + rows - 1) / rows;
    TORCH_CHECK(n * nqb * nbh < (1L << 31), "attn_fwd_split: grid too large");
    hipLaunchKernelGGL(kern, dim3(n * nqb * nbh), dim3(256), 0, cur_stream(),
                       reinterpret_cast<__hip_bfloat16*>(q.data_ptr()),
                       reinterpret_cast<__hip_bfloat16*>(k.data_ptr()),
                       reinterpret_cast<__hip_bfloat16*>(v.data_ptr()),
                       o_part.data_ptr<float>(), m_part, l_part,
                       attn_mask_ptr(mask, B, S), S, H, nbh, nqb, tps,
                       q.stride(0), q.stride(1), q.stride(2),
                       k.stride(0), k.stride(1), k.stride(2),
                       v.stride(0), v.stride(1), v.stride(2), (float)scale);
  };
  auto combine = [&](auto kern, long rows_per_block) {
    long rows = nbh * S;
    hipLaunchKernelGGL(kern,
                       dim3((rows + rows_per_block - 1) / rows_per_block),
                       dim3(256), 0, cur_stream(), o_part.data_ptr<float>(),
                       m_part, l_part,
                       reinterpret_cast<__hip_bfloat16*>(o.data_ptr()), rows,
                       (int)n);
  };
  // RB as attn_fwd picks it
  if (D == 64) {
    if (S >= 256) launch(attn_fwd_split_kernel<2, 64>, 128);
    else launch(attn_fwd_split_kernel<1, 64>, 64);
    combine(attn_fwd_combine_kernel<64>, 256 / (64 / 8));
  } else {
    if (S >= 256) launch(attn_fwd_split_kernel<2, 128>, 128);
    else launch(attn_fwd_split_kernel<1, 128>, 64);
    combine(attn_fwd_combine_kernel<128>, 256 / (128 / 8));
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

// ---- fused dropout + residual + LayerNorm (ln_drop_* kernels) ----
static bool lnd_aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

static void lnd_check_rows(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
              t.dim() >= 1 && t.is_contiguous() && lnd_aligned16(t),
              name, ": contiguous 16-byte aligned bf16 GPU tensor expected");
  long H = t.size(-1);
  TORCH_CHECK(H % 8 == 0 && H >= 8 && H <= 4096, name,
              ": the ln_drop kernels serve H % 8 == 0, 8 <= H <= 4096, got ",
              H);
  TORCH_CHECK(t.numel() / H < (1L << 31), name, ": too many rows");
}

static void lnd_check_vec(const torch::Tensor& t, long n, bool aligned,
                          const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
              t.is_contiguous() && t.numel() == n &&
              (!aligned || lnd_aligned16(t)),
              name, ": contiguous fp32 GPU tensor of ", n, " elements ",
              "expected");
}

// lane-group geometry from H / 8 vectors per row (see ln_ops.hip)
#define LND_DISPATCH(H8, CALL)                                            \
  do {                                                                    \
    if ((H8) <= 64) { CALL(64, 1); }                                      \
    else if ((H8) <= 128) { CALL(128, 1); }                               \
    else if ((H8) <= 256) { CALL(256, 1); }                               \
    else { CALL(256, 2); }                                                \
  } while (0)

static long lnd_rows_per_block(long H8) {
  return H8 <= 64 ? 4 : H8 <= 128 ? 2 : 1;
}

std::vector<torch::Tensor> ln_drop_fwd(torch::Tensor x,
                                       c10::optional<torch::Tensor> res,
                                       torch::Tensor gamma,
                                       torch::Tensor beta, double eps,
                                       double p, int64_t seed) {
  lnd_check_rows(x, "ln_drop_fwd x");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "ln_drop_fwd: 0 <= p < 1, got ", p);
  long H = x.size(-1);
  long N = x.numel() / H;
  bool has_res = res.has_value() && res->defined();
  if (has_res) {
    lnd_check_rows(*res, "ln_drop_fwd res");
    TORCH_CHECK(res->sizes() == x.sizes(), "ln_drop_fwd: res shape != x");
  }
  // gamma / beta may be views into a flat parameter buffer: any 4-byte
  // alignment is served, 16 bytes gets the float4 loads
  lnd_check_vec(gamma, H, false, "ln_drop_fwd gamma");
  lnd_check_vec(beta, H, false, "ln_drop_fwd beta");
  bool gvec = lnd_aligned16(gamma) && lnd_aligned16(beta);
  auto y = torch::empty_like(x);
  auto u = torch::empty_like(x);
  auto fopt = x.options().dtype(torch::kFloat32);
  auto mean = torch::empty({N}, fopt);
  auto rstd = torch::empty({N}, fopt);
  if (N == 0) return {y, u, mean, rstd};
  const __hip_bfloat16* rp = has_res
      ? reinterpret_cast<__hip_bfloat16*>(res->data_ptr()) : nullptr;
  long H8 = H / 8, rpb = lnd_rows_per_block(H8);
#define LND_FWD(G, V)                                                     \
  hipLaunchKernelGGL((ln_drop_fwd_kernel<G, V>), dim3((N + rpb - 1) / rpb), \
                     dim3(256), 0, cur_stream(),                          \
                     reinterpret_cast<__hip_bfloat16*>(x.data_ptr()), rp, \
                     gamma.data_ptr<float>(), beta.data_ptr<float>(),     \
                     reinterpret_cast<__hip_bfloat16*>(y.data_ptr()),     \
                     reinterpret_cast<__hip_bfloat16*>(u.data_ptr()),     \
                     mean.data_ptr<float>(), rstd.data_ptr<float>(), N,   \
                     (int)H, (float)eps, (float)p,                        \
                     (unsigned int)(uint64_t)seed, gvec)
  LND_DISPATCH(H8, LND_FWD);
#undef LND_FWD
  return {y, u, mean, rstd};
}

std::vector<torch::Tensor> ln_drop_bwd(torch::Tensor dy, torch::Tensor u,
                                       torch::Tensor gamma,
                                       torch::Tensor mean, torch::Tensor rstd,
                                       double p, int64_t seed) {
  lnd_check_rows(dy, "ln_drop_bwd dy");
  lnd_check_rows(u, "ln_drop_bwd u");
  TORCH_CHECK(u.sizes() == dy.sizes(), "ln_drop_bwd: u shape != dy");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "ln_drop_bwd: 0 <= p < 1, got ", p);
  long H = dy.size(-1);
  long N = dy.numel() / H;
  lnd_check_vec(gamma, H, false, "ln_drop_bwd gamma");
  bool gvec = lnd_aligned16(gamma);
  lnd_check_vec(mean, N, false, "ln_drop_bwd mean");
  lnd_check_vec(rstd, N, false, "ln_drop_bwd rstd");
  auto dx = torch::empty_like(dy);
  auto dres = torch::empty_like(dy);
  auto fopt = dy.options().dtype(torch::kFloat32);
  if (N == 0) {
    auto z = torch::zeros({2, H}, fopt);
    return {dx, dres, z[0], z[1]};
  }
  long H8 = H / 8, rpb = lnd_rows_per_block(H8);
  // a function of (N, H) alone: a block walks several rows, ascending
  long nb = std::min<long>((N + rpb - 1) / rpb, LND_BWD_GRID_MAX);
  auto partials = torch::empty({nb, 2, H}, fopt);
  auto gb = torch::empty({2, H}, fopt);
#define LND_BWD(G, V)                                                     \
  hipLaunchKernelGGL((ln_drop_bwd_kernel<G, V>), dim3(nb), dim3(256), 0,  \
                     cur_stream(),                                        \
                     reinterpret_cast<__hip_bfloat16*>(dy.data_ptr()),    \
                     reinterpret_cast<__hip_bfloat16*>(u.data_ptr()),     \
                     gamma.data_ptr<float>(), mean.data_ptr<float>(),     \
                     rstd.data_ptr<float>(),                              \
                     reinterpret_cast<__hip_bfloat16*>(dx.data_ptr()),    \
                     reinterpret_cast<__hip_bfloat16*>(dres.data_ptr()),  \
                     partials.data_ptr<float>(), N, (int)H, (float)p,     \
                     (unsigned int)(uint64_t)seed, gvec)
  LND_DISPATCH(H8, LND_BWD);
#undef LND_BWD
  long H2 = 2 * H;
  hipLaunchKernelGGL(ln_drop_gb_finalize_kernel,
                     dim3((H2 + LND_FIN_COLS - 1) / LND_FIN_COLS),
                     dim3(LND_FIN_COLS * LND_FIN_SLICES), 0, cur_stream(),
                     partials.data_ptr<float>(), gb.data_ptr<float>(),
                     (int)nb, (int)H2);
  return {dx, dres, gb[0], gb[1]};
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

// ---- vocab-sharded cross-entropy (ce_ops.hip) ----

// logits shard [N, V] bf16, unit column stride, row stride ld >= V
static void ce_shard_check(const torch::Tensor& logits,
                           const torch::Tensor& targets, long row_start) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 &&
              logits.scalar_type() == torch::kBFloat16,
              "ce_shard: logits must be a 2-D bf16 GPU tensor");
  long N = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 1 && V < (1L << 31), "ce_shard: 1 <= V_r < 2^31");
  TORCH_CHECK(N == 0 || (logits.stride(1) == 1 && logits.stride(0) >= V),
              "ce_shard: logits rows must be contiguous (stride(1) == 1, "
              "stride(0) >= V_r)");
  TORCH_CHECK(targets.is_cuda() && targets.scalar_type() == torch::kLong &&
              targets.dim() == 1 && targets.size(0) == N &&
              targets.is_contiguous(),
              "ce_shard: targets must be a contiguous int64 GPU vector [N]");
  TORCH_CHECK(row_start >= 0, "ce_shard: row_start must be >= 0");
}

static void ce_shard_check_rowvec(const torch::Tensor& t, long N,
                                  const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
              t.dim() == 1 && t.size(0) == N && t.is_contiguous(),
              "ce_shard: ", name, " must be a contiguous fp32 GPU vector [N]");
}

static bool ce_shard_vec_ok(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 &&
         t.stride(0) % CE_VEC == 0;
}

torch::Tensor ce_shard_stats(torch::Tensor logits, torch::Tensor targets,
                             long row_start) {
  ce_shard_check(logits, targets, row_start);
  long N = logits.size(0), V = logits.size(1);
  auto stats = torch::empty({3, N}, logits.options().dtype(torch::kFloat32));
  if (N == 0) return stats;
  TORCH_CHECK(N < (1L << 31), "ce_shard: N < 2^31");
  long ld = logits.stride(0);
  auto kern = ce_shard_vec_ok(logits) ? ce_shard_stats_kernel<true>
                                      : ce_shard_stats_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(N), dim3(256), 0, cur_stream(),
                     reinterpret_cast<__hip_bfloat16*>(logits.data_ptr()),
                     targets.data_ptr<long>(), stats.data_ptr<float>(), N, V,
                     ld, row_start);
  return stats;
}

std::vector<torch::Tensor> ce_shard_combine(torch::Tensor stats_all) {
  TORCH_CHECK(stats_all.is_cuda() && stats_all.dim() == 3 &&
              stats_all.size(0) >= 1 && stats_all.size(1) == 3 &&
              stats_all.scalar_type() == torch::kFloat32 &&
              stats_all.is_contiguous(),
              "ce_shard_combine: stats must be contiguous fp32 [world, 3, N] "
              "on the GPU");
  long world = stats_all.size(0), N = stats_all.size(2);
  auto loss_rows = torch::empty({N}, stats_all.options());
  auto lse2 = torch::empty({N}, stats_all.options());
  if (N == 0) return {loss_rows, lse2};
  hipLaunchKernelGGL(ce_shard_combine_kernel, dim3((N + 255) / 256),
                     dim3(256), 0, cur_stream(), stats_all.data_ptr<float>(),
                     loss_rows.data_ptr<float>(), lse2.data_ptr<float>(), N,
                     (int)world);
  return {loss_rows, lse2};
}

std::vector<torch::Tensor> ce_shard_bwd(torch::Tensor logits,
                                        torch::Tensor targets, long row_start,
                                        torch::Tensor lse2,
                                        torch::Tensor dloss_rows) {
  ce_shard_check(logits, targets, row_start);
  long N = logits.size(0), V = logits.size(1);
  ce_shard_check_rowvec(lse2, N, "lse2");
  ce_shard_check_rowvec(dloss_rows, N, "dloss_rows");
  auto fopt = logits.options().dtype(torch::kFloat32);
  if (N == 0)
    return {torch::empty({0, V}, logits.options()), torch::zeros({V}, fopt)};
  // dlogits keeps the logits' row stride (padding columns are never written)
  long ld = logits.stride(0);
  auto dlogits = torch::empty({N, ld}, logits.options()).slice(1, 0, V);
  long nstrips = (V + CE_STRIP_COLS - 1) / CE_STRIP_COLS;
  long nchunks = (N + CE_BWD_ROWS - 1) / CE_BWD_ROWS;
  TORCH_CHECK(nchunks <= 65535, "ce_shard_bwd: N <= 65535 * ", CE_BWD_ROWS);
  long Vpad = nstrips * CE_STRIP_COLS;
  auto partials = torch::empty({nchunks, Vpad}, fopt);
  auto dbias = torch::empty({V}, fopt);
  bool vec = ce_shard_vec_ok(logits) && ce_shard_vec_ok(dlogits) &&
             reinterpret_cast<uintptr_t>(partials.data_ptr()) % 16 == 0;
  auto kern = vec ? ce_shard_bwd_kernel<true> : ce_shard_bwd_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(nstrips, nchunks), dim3(256), 0, cur_stream(),
                     reinterpret_cast<__hip_bfloat16*>(logits.data_ptr()),
                     targets.data_ptr<long>(), lse2.data_ptr<float>(),
                     dloss_rows.data_ptr<float>(),
                     reinterpret_cast<__hip_bfloat16*>(dlogits.data_ptr()),
                     partials.data_ptr<float>(), N, V, ld, row_start, Vpad);
  hipLaunchKernelGGL(ce_shard_dbias_kernel, dim3((V + 255) / 256), dim3(256),
                     0, cur_stream(), partials.data_ptr<float>(),
                     dbias.data_ptr<float>(), V, Vpad, nchunks);
  return {dlogits, dbias};
}

// ---- projected-LSTM cell kernels (lstm_ops.hip) ----

// [rows, cols] matrix of `dtype` on the GPU: unit column stride, row stride
// >= cols, base and rows 16-byte aligned
static void lstmp_check_mat(const torch::Tensor& t, long rows, long cols,
                            torch::ScalarType dtype, bool strided_rows,
                            const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 2 && t.scalar_type() == dtype &&
                  t.size(0) == rows && t.size(1) == cols,
              "lstmp: ", name, " must be a [", rows, ", ", cols, "] ",
              dtype, " GPU tensor, got ", t.sizes(), " ", t.scalar_type());
  TORCH_CHECK(t.stride(1) == 1 && t.stride(0) >= cols,
              "lstmp: ", name, " needs a contiguous last dimension");
  TORCH_CHECK(strided_rows || t.stride(0) == cols || rows == 1,
              "lstmp: ", name, " must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 &&
                  (rows == 1 || t.stride(0) * t.element_size() % 16 == 0),
              "lstmp: ", name, " rows must be 16-byte aligned");
}

static void lstmp_check_dims(long B, long H, long P) {
  TORCH_CHECK(B >= 1 && B <= (1L << 20), "lstmp: 1 <= B <= 2^20, got ", B);
  TORCH_CHECK(P >= 32 && P % 32 == 0 && P <= LSTMP_MAX_P,
              "lstmp: P must be a multiple of 32 in [32, ", LSTMP_MAX_P,
              "], got ", P);
  TORCH_CHECK(H >= 16 && H % 16 == 0 && H <= (1L << 20),
              "lstmp: H must be a multiple of 16 (at most 2^20), got ", H);
}

#define LSTMP_S(t) reinterpret_cast<short*>((t).data_ptr())

// One forward step: (gx_t [B, 4H] bf16 row-strided, h_prev [B, P] bf16
// row-strided, w_hh [4H, P] bf16, bias [4H] fp32, c_prev [B, H] fp32) ->
// writes c_out [B, H] fp32, hc_out [B, H] bf16, gates_out [B, 4H] bf16.
void lstmp_cell_fwd(torch::Tensor gx, torch::Tensor h_prev, torch::Tensor w_hh,
                    torch::Tensor bias, torch::Tensor c_prev,
                    torch::Tensor c_out, torch::Tensor hc_out,
                    torch::Tensor gates_out) {
  TORCH_CHECK(h_prev.dim() == 2 && c_prev.dim() == 2,
              "lstmp_cell_fwd: h_prev [B, P] and c_prev [B, H] expected");
  long B = h_prev.size(0), P = h_prev.size(1), H = c_prev.size(1);
  lstmp_check_dims(B, H, P);
  lstmp_check_mat(gx, B, 4 * H, torch::kBFloat16, true, "gx_t");
  lstmp_check_mat(h_prev, B, P, torch::kBFloat16, true, "h_prev");
  lstmp_check_mat(w_hh, 4 * H, P, torch::kBFloat16, false, "w_hh");
  lstmp_check_mat(c_prev, B, H, torch::kFloat32, false, "c_prev");
  lstmp_check_mat(c_out, B, H, torch::kFloat32, false, "c_out");
  lstmp_check_mat(hc_out, B, H, torch::kBFloat16, false, "hc_out");
  lstmp_check_mat(gates_out, B, 4 * H, torch::kBFloat16, false, "gates_out");
  TORCH_CHECK(bias.is_cuda() && bias.scalar_type() == torch::kFloat32 &&
                  bias.dim() == 1 && bias.size(0) == 4 * H &&
                  bias.is_contiguous(),
              "lstmp_cell_fwd: bias must be a contiguous fp32 GPU vector [4H]");
  dim3 grid((H + LSTMP_TILE_H - 1) / LSTMP_TILE_H,
            (B + LSTMP_TILE_B - 1) / LSTMP_TILE_B);
  hipLaunchKernelGGL(lstmp_cell_fwd_kernel, grid, dim3(256),
                     lstmp_lds_bytes((int)P, true), cur_stream(), LSTMP_S(gx),
                     gx.stride(0), LSTMP_S(h_prev), h_prev.stride(0),
                     LSTMP_S(w_hh), bias.data_ptr<float>(),
                     c_prev.data_ptr<float>(), c_out.data_ptr<float>(),
                     LSTMP_S(hc_out), LSTMP_S(gates_out), (int)B, (int)H,
                     (int)P);
}

// One backward step: (dh_t [B, P] bf16 row-strided, w_hr [P, H] bf16, gates
// [B, 4H] bf16, c_t, c_prev [B, H] fp32, dc_next [B, H] fp32 or None = 0) ->
// writes dgates [B, 4H] bf16 row-strided and dc_prev [B, H] fp32. dc_prev
// may be dc_next itself (each element is read and written by one lane).
void lstmp_cell_bwd(torch::Tensor dh, torch::Tensor w_hr, torch::Tensor gates,
                    torch::Tensor c_t, torch::Tensor c_prev,
                    c10::optional<torch::Tensor> dc_next, torch::Tensor dgates,
                    torch::Tensor dc_prev) {
  TORCH_CHECK(dh.dim() == 2 && c_t.dim() == 2,
              "lstmp_cell_bwd: dh_t [B, P] and c_t [B, H] expected");
  long B = dh.size(0), P = dh.size(1), H = c_t.size(1);
  lstmp_check_dims(B, H, P);
  lstmp_check_mat(dh, B, P, torch::kBFloat16, true, "dh_t");
  lstmp_check_mat(w_hr, P, H, torch::kBFloat16, false, "w_hr");
  lstmp_check_mat(gates, B, 4 * H, torch::kBFloat16, false, "gates");
  lstmp_check_mat(c_t, B, H, torch::kFloat32, false, "c_t");
  lstmp_check_mat(c_prev, B, H, torch::kFloat32, false, "c_prev");
  lstmp_check_mat(dgates, B, 4 * H, torch::kBFloat16, true, "dgates");
  lstmp_check_mat(dc_prev, B, H, torch::kFloat32, false, "dc_prev");
  const float* dcn = nullptr;
  if (dc_next.has_value() && dc_next->defined()) {
    lstmp_check_mat(*dc_next, B, H, torch::kFloat32, false, "dc_next");
    dcn = dc_next->data_ptr<float>();
  }
  dim3 grid((H + LSTMP_TILE_H - 1) / LSTMP_TILE_H,
            (B + LSTMP_TILE_B - 1) / LSTMP_TILE_B);
  hipLaunchKernelGGL(lstmp_cell_bwd_kernel, grid, dim3(256),
                     lstmp_lds_bytes((int)P, false), cur_stream(), LSTMP_S(dh),
                     dh.stride(0), LSTMP_S(w_hr), LSTMP_S(gates),
                     c_t.data_ptr<float>(), c_prev.data_ptr<float>(), dcn,
                     LSTMP_S(dgates), dgates.stride(0),
                     dc_prev.data_ptr<float>(), (int)B, (int)H, (int)P);
}
#undef LSTMP_S

// ---- sampled softmax loss (ssm_ops.hip) ----

// contiguous [rows, cols] GPU matrix of `dtype`, base and rows 16-byte aligned
static void ssm_check_mat(const torch::Tensor& t, long rows, long cols,
                          torch::ScalarType dtype, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 2 && t.scalar_type() == dtype &&
                  t.size(0) == rows && t.size(1) == cols,
              "ssm: ", name, " must be a [", rows, ", ", cols, "] ", dtype,
              " GPU tensor, got ", t.sizes(), " ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), "ssm: ", name, " must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0 &&
                  cols * t.element_size() % 16 == 0,
              "ssm: ", name, " rows must be 16-byte aligned");
}

static void ssm_check_vec(const torch::Tensor& t, long n,
                          torch::ScalarType dtype, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 1 && t.size(0) == n &&
                  t.scalar_type() == dtype && t.is_contiguous(),
              "ssm: ", name, " must be a contiguous ", dtype,
              " GPU vector [", n, "], got ", t.sizes(), " ", t.scalar_type());
}

static void ssm_check_dims(long N, long S, long P) {
  TORCH_CHECK(P >= 32 && P % 32 == 0 && P <= SSM_MAX_P,
              "ssm: P must be a multiple of 32 in [32, ", SSM_MAX_P,
              "], got ", P);
  TORCH_CHECK(S >= 1 && S <= (1L << 24), "ssm: 1 <= S <= 2^24, got ", S);
  TORCH_CHECK(N >= 1 && N <= (1L << 24), "ssm: 1 <= N <= 2^24, got ", N);
}

static long ssm_pad(long S) { return (S + SSM_BN - 1) / SSM_BN * SSM_BN; }

#define SSM_S(t) reinterpret_cast<short*>((t).data_ptr())

// (table [V, P] fp32 or bf16, bias [V] fp32 or None, sampled [S], targets
// [N], logq_samp [S], logq_true [N]) -> Wg [S_pad, P] bf16, Wt [N, P] bf16,
// off [S_pad], off0 [N]. Ids within [0, V) are the caller's contract.
std::vector<torch::Tensor> ssm_prep(torch::Tensor table,
                                    c10::optional<torch::Tensor> bias,
                                    torch::Tensor sampled,
                                    torch::Tensor targets,
                                    torch::Tensor logq_samp,
                                    torch::Tensor logq_true) {
  TORCH_CHECK(table.dim() == 2 && sampled.dim() == 1 && targets.dim() == 1,
              "ssm_prep: table [V, P], sampled [S], targets [N] expected");
  long V = table.size(0), P = table.size(1);
  long S = sampled.size(0), N = targets.size(0);
  ssm_check_dims(N, S, P);
  TORCH_CHECK(V >= 1 && V < (1L << 31), "ssm_prep: 1 <= V < 2^31");
  bool f32 = table.scalar_type() == torch::kFloat32;
  ssm_check_mat(table, V, P, f32 ? torch::kFloat32 : torch::kBFloat16,
                "table (fp32 or bf16)");
  ssm_check_vec(sampled, S, torch::kLong, "sampled");
  ssm_check_vec(targets, N, torch::kLong, "targets");
  ssm_check_vec(logq_samp, S, torch::kFloat32, "logq_samp");
  ssm_check_vec(logq_true, N, torch::kFloat32, "logq_true");
  const float* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    ssm_check_vec(*bias, V, torch::kFloat32, "bias");
    bp = bias->data_ptr<float>();
  }
  long S_pad = ssm_pad(S);
  auto bopt = table.options().dtype(torch::kBFloat16);
  auto fopt = table.options().dtype(torch::kFloat32);
  auto wg = torch::empty({S_pad, P}, bopt), wt = torch::empty({N, P}, bopt);
  auto off = torch::empty({S_pad}, fopt), off0 = torch::empty({N}, fopt);
  long items = (S_pad + N) * (P / 8);
  dim3 grid((unsigned)((items + 255) / 256));
#define SSM_PREP_ARGS                                                      \
  bp, sampled.data_ptr<long>(), targets.data_ptr<long>(),                  \
      logq_samp.data_ptr<float>(), logq_true.data_ptr<float>(), SSM_S(wg), \
      SSM_S(wt), off.data_ptr<float>(), off0.data_ptr<float>(), (int)S,    \
      (int)S_pad, (int)N, (int)P
  if (f32)
    hipLaunchKernelGGL(ssm_prep_kernel<float>, grid, dim3(256), 0,
                       cur_stream(), table.data_ptr<float>(), SSM_PREP_ARGS);
  else
    hipLaunchKernelGGL(ssm_prep_kernel<short>, grid, dim3(256), 0,
                       cur_stream(), SSM_S(table), SSM_PREP_ARGS);
#undef SSM_PREP_ARGS
  return {wg, wt, off, off0};
}

// shared operand checks of the forward and the backward; returns S_pad
static long ssm_check_main(const torch::Tensor& h, const torch::Tensor& wg,
                           const torch::Tensor& off,
                           const torch::Tensor& sampled,
                           const torch::Tensor& targets) {
  TORCH_CHECK(h.dim() == 2 && sampled.dim() == 1,
              "ssm: h [N, P] and sampled [S] expected");
  long N = h.size(0), P = h.size(1), S = sampled.size(0);
  ssm_check_dims(N, S, P);
  long S_pad = ssm_pad(S);
  ssm_check_mat(h, N, P, torch::kBFloat16, "h");
  ssm_check_mat(wg, S_pad, P, torch::kBFloat16, "Wg");
  ssm_check_vec(off, S_pad, torch::kFloat32, "off");
  ssm_check_vec(sampled, S, torch::kLong, "sampled");
  ssm_check_vec(targets, N, torch::kLong, "targets");
  return S_pad;
}

// -> loss [N], lse2 [N] (log2 domain), z0 [N], all fp32
std::vector<torch::Tensor> ssm_fwd(torch::Tensor h, torch::Tensor wg,
                                   torch::Tensor wt, torch::Tensor off,
                                   torch::Tensor off0, torch::Tensor sampled,
                                   torch::Tensor targets) {
  long S_pad = ssm_check_main(h, wg, off, sampled, targets);
  long N = h.size(0), P = h.size(1), S = sampled.size(0);
  ssm_check_mat(wt, N, P, torch::kBFloat16, "Wt");
  ssm_check_vec(off0, N, torch::kFloat32, "off0");
  long splits = (S_pad + SSM_SPLIT_COLS - 1) / SSM_SPLIT_COLS;
  auto fopt = h.options().dtype(torch::kFloat32);
  auto part = torch::empty({splits, N, 2}, fopt);
  auto loss = torch::empty({N}, fopt), lse2 = torch::empty({N}, fopt);
  auto z0 = torch::empty({N}, fopt);
  dim3 grid((unsigned)((N + SSM_BM - 1) / SSM_BM), (unsigned)splits);
  hipLaunchKernelGGL(ssm_fwd_kernel, grid, dim3(256), 0, cur_stream(),
                     SSM_S(h), SSM_S(wg), SSM_S(wt), off.data_ptr<float>(),
                     off0.data_ptr<float>(), sampled.data_ptr<long>(),
                     targets.data_ptr<long>(), part.data_ptr<float>(),
                     z0.data_ptr<float>(), (int)N, (int)S, (int)S_pad, (int)P);
  hipLaunchKernelGGL(ssm_combine_kernel, dim3((unsigned)((N + 255) / 256)),
                     dim3(256), 0, cur_stream(), part.data_ptr<float>(),
                     z0.data_ptr<float>(), loss.data_ptr<float>(),
                     lse2.data_ptr<float>(), (int)N, (int)splits);
  return {loss, lse2, z0};
}

// g [N] is the incoming gradient of loss -> dz [N, S_pad] bf16, dz0 [N] fp32,
// db_samp [S] fp32 (column sums of the unrounded dz)
std::vector<torch::Tensor> ssm_bwd(torch::Tensor h, torch::Tensor wg,
                                   torch::Tensor off, torch::Tensor sampled,
                                   torch::Tensor targets, torch::Tensor lse2,
                                   torch::Tensor z0, torch::Tensor g) {
  long S_pad = ssm_check_main(h, wg, off, sampled, targets);
  long N = h.size(0), P = h.size(1), S = sampled.size(0);
  ssm_check_vec(lse2, N, torch::kFloat32, "lse2");
  ssm_check_vec(z0, N, torch::kFloat32, "z0");
  ssm_check_vec(g, N, torch::kFloat32, "g");
  long splits = (S_pad + SSM_SPLIT_COLS - 1) / SSM_SPLIT_COLS;
  long row_blocks = (N + SSM_BM - 1) / SSM_BM;
  auto fopt = h.options().dtype(torch::kFloat32);
  auto dz = torch::empty({N, S_pad}, h.options());
  auto colpart = torch::empty({row_blocks, S_pad}, fopt);
  auto dz0 = torch::empty({N}, fopt), db = torch::empty({S}, fopt);
  hipLaunchKernelGGL(ssm_bwd_kernel, dim3((unsigned)row_blocks,
                                          (unsigned)splits),
                     dim3(256), 0, cur_stream(), SSM_S(h), SSM_S(wg),
                     off.data_ptr<float>(), sampled.data_ptr<long>(),
                     targets.data_ptr<long>(), lse2.data_ptr<float>(),
                     z0.data_ptr<float>(), g.data_ptr<float>(), SSM_S(dz),
                     colpart.data_ptr<float>(), dz0.data_ptr<float>(), (int)N,
                     (int)S, (int)S_pad, (int)P);
  hipLaunchKernelGGL(ssm_dbias_kernel, dim3((unsigned)((S + 255) / 256)),
                     dim3(256), 0, cur_stream(), colpart.data_ptr<float>(),
                     db.data_ptr<float>(), (int)S, (int)S_pad,
                     (int)row_blocks);
  return {dz, dz0, db};
}
#undef SSM_S

// ---- fused linear + cross-entropy (lce_ops.hip) ----

static void lce_check_vec(const torch::Tensor& t, long n,
                          torch::ScalarType dtype, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 1 && t.size(0) == n &&
                  t.scalar_type() == dtype && t.is_contiguous(),
              "lce: ", name, " must be a contiguous ", dtype,
              " GPU vector [", n, "], got ", t.sizes(), " ", t.scalar_type());
}

// contiguous [rows, K] bf16 GPU matrix, base 16-byte aligned, K in range
static void lce_check_mat(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 2 &&
                  t.scalar_type() == torch::kBFloat16,
              "lce: ", name, " must be a 2-d bf16 GPU tensor, got ", t.sizes(),
              " ", t.scalar_type());
  long K = t.size(1);
  TORCH_CHECK(K >= 32 && K % 32 == 0 && K <= LCE_MAX_K,
              "lce: K must be a multiple of 32 in [32, ", LCE_MAX_K,
              "], got ", K);
  TORCH_CHECK(t.is_contiguous(), "lce: ", name, " must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "lce: ",
              name, " must be 16-byte aligned");
}

#define LCE_S(t) reinterpret_cast<short*>((t).data_ptr())

// (h [N, K] bf16, labels [N] int64, ignore_index, M_cap) -> Hc [M_cap, K]
// bf16, rows [M_cap] int64 (-1 pad), tgt [M_cap] int32 (-1 pad), count [1]
// int32 on the device
std::vector<torch::Tensor> lce_compact(torch::Tensor h, torch::Tensor labels,
                                       long ignore_index, long M_cap) {
  lce_check_mat(h, "h");
  long N = h.size(0), K = h.size(1);
  TORCH_CHECK(N >= 1 && N <= (1L << 24), "lce: 1 <= N <= 2^24, got ", N);
  TORCH_CHECK(M_cap >= 1 && M_cap <= N, "lce: 1 <= M_cap <= N, got ", M_cap);
  TORCH_CHECK(labels.scalar_type() == torch::kLong,
              "lce: labels must be int64, got ", labels.scalar_type());
  lce_check_vec(labels, N, torch::kLong, "labels");
  auto hc = torch::empty({M_cap, K}, h.options());
  auto rows = torch::empty({M_cap}, labels.options());
  auto tgt = torch::empty({M_cap}, labels.options().dtype(torch::kInt32));
  auto count = torch::empty({1}, labels.options().dtype(torch::kInt32));
  hipLaunchKernelGGL(lce_scan_kernel, dim3(1), dim3(256), 0, cur_stream(),
                     labels.data_ptr<long>(), ignore_index, (int)N, (int)M_cap,
                     rows.data_ptr<long>(), tgt.data_ptr<int>(),
                     count.data_ptr<int>());
  long items = M_cap * (K / 8);
  hipLaunchKernelGGL(lce_gather_kernel, dim3((unsigned)((items + 255) / 256)),
                     dim3(256), 0, cur_stream(), LCE_S(h),
                     rows.data_ptr<long>(), LCE_S(hc), (int)M_cap, (int)K);
  return {hc, rows, tgt, count};
}

// shared operand checks of the forward and the backward; returns the bias
// pointer (null without a bias)
static const float* lce_check_main(const torch::Tensor& hc,
                                   const torch::Tensor& w,
                                   const c10::optional<torch::Tensor>& bias,
                                   const torch::Tensor& rows,
                                   const torch::Tensor& tgt,
                                   const torch::Tensor& count) {
  lce_check_mat(hc, "Hc");
  lce_check_mat(w, "weight");
  long M_cap = hc.size(0), V = w.size(0);
  TORCH_CHECK(w.size(1) == hc.size(1), "lce: weight must be [V, ", hc.size(1),
              "], got ", w.sizes());
  TORCH_CHECK(V >= 2 && V < (1L << 30), "lce: 2 <= V < 2^30, got ", V);
  TORCH_CHECK(M_cap >= 1 && M_cap <= (1L << 24),
              "lce: 1 <= M_cap <= 2^24, got ", M_cap);
  lce_check_vec(rows, M_cap, torch::kLong, "rows");
  lce_check_vec(tgt, M_cap, torch::kInt32, "tgt");
  lce_check_vec(count, 1, torch::kInt32, "count");
  if (bias.has_value() && bias->defined()) {
    lce_check_vec(*bias, V, torch::kFloat32, "bias");
    return bias->data_ptr<float>();
  }
  return nullptr;
}

// (Hc, weight [V, K] bf16, bias [V] fp32 or None, rows, tgt, count, N) ->
// loss [N] fp32 (zeros in rows that were not kept), stats [2] = (sum, mean
// over the kept rows), lse2 [M_cap] (log2 domain)
std::vector<torch::Tensor> lce_fwd(torch::Tensor hc, torch::Tensor w,
                                   c10::optional<torch::Tensor> bias,
                                   torch::Tensor rows, torch::Tensor tgt,
                                   torch::Tensor count, long N) {
  const float* bp = lce_check_main(hc, w, bias, rows, tgt, count);
  long M_cap = hc.size(0), K = hc.size(1), V = w.size(0);
  TORCH_CHECK(N >= M_cap, "lce_fwd: N must be at least M_cap");
  long splits = (V + LCE_SPLIT_COLS - 1) / LCE_SPLIT_COLS;
  long row_blocks = (M_cap + LCE_BM - 1) / LCE_BM;
  long cblocks = (M_cap + 255) / 256;
  auto fopt = hc.options().dtype(torch::kFloat32);
  auto part = torch::empty({splits, M_cap, 2}, fopt);
  // a target outside [0, V) is picked by no lane: its row's loss is NaN
  auto zt = torch::full({M_cap}, std::numeric_limits<float>::quiet_NaN(), fopt);
  auto loss = torch::zeros({N}, fopt);
  auto lse2 = torch::empty({M_cap}, fopt);
  auto blocksum = torch::empty({cblocks}, fopt);
  auto stats = torch::empty({2}, fopt);
  hipLaunchKernelGGL(lce_fwd_kernel,
                     dim3((unsigned)row_blocks, (unsigned)splits), dim3(256),
                     0, cur_stream(), LCE_S(hc), LCE_S(w), bp,
                     tgt.data_ptr<int>(), count.data_ptr<int>(),
                     part.data_ptr<float>(), zt.data_ptr<float>(), (int)M_cap,
                     (int)V, (int)K);
  hipLaunchKernelGGL(lce_combine_kernel, dim3((unsigned)cblocks), dim3(256),
                     0, cur_stream(), part.data_ptr<float>(),
                     zt.data_ptr<float>(), rows.data_ptr<long>(),
                     count.data_ptr<int>(), loss.data_ptr<float>(),
                     lse2.data_ptr<float>(), blocksum.data_ptr<float>(),
                     (int)M_cap, (int)splits);
  hipLaunchKernelGGL(lce_mean_kernel, dim3(1), dim3(256), 0, cur_stream(),
                     blocksum.data_ptr<float>(), count.data_ptr<int>(),
                     stats.data_ptr<float>(), (int)cblocks);
  return {loss, stats, lse2};
}

// g_rows [N] fp32 (gradient of the loss rows) and / or g_mean [1] fp32
// (gradient of the mean) -> dz [M_cap, V_ld] bf16, db [V] fp32 (column sums
// of the unrounded dz; undefined without a bias)
std::vector<torch::Tensor> lce_bwd(torch::Tensor hc, torch::Tensor w,
                                   c10::optional<torch::Tensor> bias,
                                   torch::Tensor rows, torch::Tensor tgt,
                                   torch::Tensor count, torch::Tensor lse2,
                                   c10::optional<torch::Tensor> g_rows,
                                   c10::optional<torch::Tensor> g_mean) {
  const float* bp = lce_check_main(hc, w, bias, rows, tgt, count);
  long M_cap = hc.size(0), K = hc.size(1), V = w.size(0);
  lce_check_vec(lse2, M_cap, torch::kFloat32, "lse2");
  const float* grp = nullptr;
  const float* gmp = nullptr;
  if (g_rows.has_value() && g_rows->defined()) {
    TORCH_CHECK(g_rows->dim() == 1 && g_rows->size(0) >= M_cap,
                "lce_bwd: g_rows must be [N] with N >= M_cap");
    lce_check_vec(*g_rows, g_rows->size(0), torch::kFloat32, "g_rows");
    grp = g_rows->data_ptr<float>();
  }
  if (g_mean.has_value() && g_mean->defined()) {
    lce_check_vec(*g_mean, 1, torch::kFloat32, "g_mean");
    gmp = g_mean->data_ptr<float>();
  }
  long V_ld = (V + 7) / 8 * 8;
  long splits = (V + LCE_SPLIT_COLS - 1) / LCE_SPLIT_COLS;
  long row_blocks = (M_cap + LCE_BM - 1) / LCE_BM;
  auto fopt = hc.options().dtype(torch::kFloat32);
  auto dz = torch::empty({M_cap, V_ld}, hc.options());
  torch::Tensor colpart, db;
  if (bp) {
    colpart = torch::empty({row_blocks, V_ld}, fopt);
    db = torch::empty({V}, fopt);
  }
  hipLaunchKernelGGL(lce_bwd_kernel,
                     dim3((unsigned)row_blocks, (unsigned)splits), dim3(256),
                     0, cur_stream(), LCE_S(hc), LCE_S(w), bp,
                     tgt.data_ptr<int>(), count.data_ptr<int>(),
                     lse2.data_ptr<float>(), rows.data_ptr<long>(), grp, gmp,
                     LCE_S(dz), bp ? colpart.data_ptr<float>() : nullptr,
                     (int)M_cap, (int)V, (int)V_ld, (int)K);
  if (bp)
    hipLaunchKernelGGL(lce_dbias_kernel, dim3((unsigned)((V + 255) / 256)),
                       dim3(256), 0, cur_stream(), colpart.data_ptr<float>(),
                       count.data_ptr<int>(), db.data_ptr<float>(), (int)V,
                       (int)V_ld, (int)row_blocks);
  return {dz, db};
}
#undef LCE_S

// ---- fused NeuMF (ncf_ops.hip) ----

static void neumf_check_f32(const torch::Tensor& t, const torch::Tensor& ids,
                            const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == ids.device() &&
                  t.scalar_type() == torch::kFloat32 && t.is_contiguous(),
              "neumf: ", name, " must be a contiguous fp32 tensor on the ids' "
              "GPU, got ", t.sizes(), " ", t.scalar_type());
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "neumf: ",
              name, " must be 16-byte aligned");
}

static void neumf_check_width(long w, const char* name) {
  TORCH_CHECK(w >= 8 && w <= NEUMF_MAX_WIDTH && w % 8 == 0, "neumf: ", name,
              " must be a multiple of 8 in [8, ", NEUMF_MAX_WIDTH, "], got ",
              w);
}

static const float* neumf_opt_rows(const c10::optional<torch::Tensor>& t,
                                   const torch::Tensor& ids,
                                   const char* name) {
  if (!t.has_value() || !t->defined()) return nullptr;
  neumf_check_f32(*t, ids, name);
  TORCH_CHECK(t->dim() == 1 && t->size(0) == ids.size(0), "neumf: ", name,
              " must be [B]");
  return t->data_ptr<float>();
}

// Checks every operand and fills the kernel arguments; nothing is launched
// when a check fails. tables = (mf_user, mf_item, mlp_user, mlp_item).
static NeumfArgs neumf_args(const torch::Tensor& users,
                            const torch::Tensor& items,
                            const std::vector<torch::Tensor>& tables,
                            const std::vector<torch::Tensor>& weights,
                            const std::vector<torch::Tensor>& biases,
                            const torch::Tensor& w_head,
                            const torch::Tensor& b_head,
                            const c10::optional<torch::Tensor>& labels,
                            const c10::optional<torch::Tensor>& weight) {
  TORCH_CHECK(users.is_cuda() && users.dim() == 1 &&
                  users.scalar_type() == torch::kLong &&
                  users.is_contiguous() && items.is_cuda() &&
                  items.device() == users.device() && items.dim() == 1 &&
                  items.scalar_type() == torch::kLong &&
                  items.is_contiguous() && items.size(0) == users.size(0),
              "neumf: users and items must be contiguous int64 GPU vectors of "
              "one length");
  long B = users.size(0);
  TORCH_CHECK(B >= 1 && B <= (1L << 30), "neumf: 1 <= B <= 2^30, got ", B);
  TORCH_CHECK(tables.size() == 4, "neumf: four tables expected");
  const char* tn[4] = {"mf_user", "mf_item", "mlp_user", "mlp_item"};
  for (int i = 0; i < 4; ++i) {
    neumf_check_f32(tables[i], users, tn[i]);
    TORCH_CHECK(tables[i].dim() == 2 && tables[i].size(0) >= 1 &&
                    tables[i].size(0) < (1L << 31),
                "neumf: ", tn[i], " must be [rows, D] with 1 <= rows < 2^31");
  }
  long mf = tables[0].size(1), E = tables[2].size(1);
  TORCH_CHECK(tables[1].size(1) == mf && tables[3].size(1) == E &&
                  tables[2].size(0) == tables[0].size(0) &&
                  tables[3].size(0) == tables[1].size(0),
              "neumf: the user tables and the item tables must agree in rows, "
              "the mf tables and the mlp tables in width");
  neumf_check_width(mf, "mf_dim");
  neumf_check_width(2 * E, "the MLP input width");
  long L = (long)weights.size();
  TORCH_CHECK(L >= 1 && L <= NEUMF_MAX_LAYERS && (long)biases.size() == L,
              "neumf: 1 to ", NEUMF_MAX_LAYERS,
              " MLP layers with a bias each expected, got ", L);
  NeumfArgs a = {};
  a.users = users.data_ptr<long>();
  a.items = items.data_ptr<long>();
  a.mf_user = tables[0].data_ptr<float>();
  a.mf_item = tables[1].data_ptr<float>();
  a.mlp_user = tables[2].data_ptr<float>();
  a.mlp_item = tables[3].data_ptr<float>();
  a.num_users = tables[0].size(0);
  a.num_items = tables[1].size(0);
  a.B = (int)B;
  a.mf = (int)mf;
  a.E = (int)E;
  a.L = (int)L;
  NeumfLayer* ls[NEUMF_MAX_LAYERS] = {&a.l1, &a.l2, &a.l3, &a.l4};
  long K = 2 * E, act = 0, P = 0;
  for (long l = 0; l < L; ++l) {
    const torch::Tensor& W = weights[l];
    neumf_check_f32(W, users, "an MLP weight");
    neumf_check_f32(biases[l], users, "an MLP bias");
    TORCH_CHECK(W.dim() == 2 && W.size(1) == K && biases[l].dim() == 1 &&
                    biases[l].size(0) == W.size(0),
                "neumf: MLP layer ", l + 1, " must be [N, ", K,
                "] with bias [N], got ", W.sizes(), " and ",
                biases[l].sizes());
    long N = W.size(0);
    neumf_check_width(N, "an MLP width");
    NeumfLayer& ly = *ls[l];
    ly.W = W.data_ptr<float>();
    ly.b = biases[l].data_ptr<float>();
    ly.K = (int)K;
    ly.N = (int)N;
    ly.in_off = (int)(act - K);  // column of H_{l-1}; unused for l = 1
    ly.out_off = (int)act;
    ly.w_off = (int)P;
    ly.b_off = (int)(P + N * K);
    P += N * K + N;
    act += N;
    K = N;
  }
  a.l1.in_off = 0;
  a.act_ld = (int)act;
  a.wl = (int)K;
  a.act_off_last = (int)(act - K);
  a.head_off = (int)P;
  a.P = (int)(P + mf + K + 1);
  neumf_check_f32(w_head, users, "the head weight");
  neumf_check_f32(b_head, users, "the head bias");
  TORCH_CHECK(w_head.numel() == mf + K && b_head.numel() == 1,
              "neumf: the head must be [1, ", mf + K, "] with one bias, got ",
              w_head.sizes());
  a.w_head = w_head.data_ptr<float>();
  a.b_head = b_head.data_ptr<float>();
  a.labels = neumf_opt_rows(labels, users, "labels");
  a.weight = neumf_opt_rows(weight, users, "weight");
  TORCH_CHECK(a.labels || !a.weight, "neumf: weight needs labels");
  return a;
}

// (users [B], items [B], tables, MLP weights, MLP biases, head weight, head
// bias, labels [B] or None, weight [B] or None, save_acts) -> (logits [B],
// loss_rows [B] (empty without labels), acts [B, sum N_l] (empty unless
// save_acts): the post-ReLU activations neumf_bwd reads)
std::vector<torch::Tensor> neumf_fwd(torch::Tensor users, torch::Tensor items,
                                     std::vector<torch::Tensor> tables,
                                     std::vector<torch::Tensor> weights,
                                     std::vector<torch::Tensor> biases,
                                     torch::Tensor w_head, torch::Tensor b_head,
                                     c10::optional<torch::Tensor> labels,
                                     c10::optional<torch::Tensor> weight,
                                     bool save_acts) {
  NeumfArgs a = neumf_args(users, items, tables, weights, biases, w_head,
                           b_head, labels, weight);
  auto fopt = w_head.options();
  auto logits = torch::empty({a.B}, fopt);
  auto loss = torch::empty({a.labels ? a.B : 0}, fopt);
  auto acts = torch::empty({save_acts ? a.B : 0, a.act_ld}, fopt);
  unsigned tiles = (unsigned)((a.B + NEUMF_TILE - 1) / NEUMF_TILE);
  hipLaunchKernelGGL(neumf_fwd_kernel, dim3(tiles), dim3(256), 0,
                     cur_stream(), a, logits.data_ptr<float>(),
                     a.labels ? loss.data_ptr<float>() : nullptr,
                     save_acts ? acts.data_ptr<float>() : nullptr);
  return {logits, loss, acts};
}

// (..., logits, acts of neumf_fwd, labels, weight, g_logits [B] or None,
// g_loss [B] or None) -> (d_mf_user [B, mf], d_mf_item [B, mf], d_mlp_user
// [B, E], d_mlp_item [B, E]: one row per sample, and the dense gradients as
// one vector [P]: per layer dW_l [N_l, K_l] then db_l [N_l], then dw_head
// [mf + N_L], db_head [1])
std::vector<torch::Tensor> neumf_bwd(torch::Tensor users, torch::Tensor items,
                                     std::vector<torch::Tensor> tables,
                                     std::vector<torch::Tensor> weights,
                                     std::vector<torch::Tensor> biases,
                                     torch::Tensor w_head, torch::Tensor b_head,
                                     torch::Tensor logits, torch::Tensor acts,
                                     c10::optional<torch::Tensor> labels,
                                     c10::optional<torch::Tensor> weight,
                                     c10::optional<torch::Tensor> g_logits,
                                     c10::optional<torch::Tensor> g_loss) {
  NeumfArgs a = neumf_args(users, items, tables, weights, biases, w_head,
                           b_head, labels, weight);
  const float* zl = neumf_opt_rows(logits, users, "logits");
  const float* gz = neumf_opt_rows(g_logits, users, "g_logits");
  const float* gl = neumf_opt_rows(g_loss, users, "g_loss");
  TORCH_CHECK(zl, "neumf_bwd: logits expected");
  neumf_check_f32(acts, users, "acts");
  TORCH_CHECK(acts.dim() == 2 && acts.size(0) == a.B &&
                  acts.size(1) == a.act_ld,
              "neumf_bwd: acts must be [", a.B, ", ", a.act_ld, "], got ",
              acts.sizes());
  auto fopt = w_head.options();
  auto d_mfu = torch::empty({a.B, a.mf}, fopt);
  auto d_mfi = torch::empty({a.B, a.mf}, fopt);
  auto d_mlpu = torch::empty({a.B, a.E}, fopt);
  auto d_mlpi = torch::empty({a.B, a.E}, fopt);
  int tiles = (a.B + NEUMF_TILE - 1) / NEUMF_TILE;
  int blocks = std::min(tiles, NEUMF_MAX_BWD_BLOCKS);
  auto ws = torch::empty({blocks, a.P}, fopt);
  auto dense = torch::empty({a.P}, fopt);
  hipLaunchKernelGGL(neumf_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     cur_stream(), a, zl, acts.data_ptr<float>(), gz, gl,
                     d_mfu.data_ptr<float>(), d_mfi.data_ptr<float>(),
                     d_mlpu.data_ptr<float>(), d_mlpi.data_ptr<float>(),
                     ws.data_ptr<float>(), tiles);
  hipLaunchKernelGGL(neumf_reduce_kernel, dim3((unsigned)((a.P + 255) / 256)),
                     dim3(256), 0, cur_stream(), ws.data_ptr<float>(),
                     dense.data_ptr<float>(), a.P, blocks);
  return {d_mfu, d_mfi, d_mlpu, d_mlpi, dense};
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
  m.def("coalesce_rows_ranked", &coalesce_rows_ranked,
        "sort-free deterministic coalesce of row-sparse gradients: "
        "(uniq[n], out[n, D], count[1]), padded, no host read");
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
  m.def("ce_shard_stats", &ce_shard_stats,
        "vocab-sharded CE: (logits [N, V_r] bf16, targets, row_start) -> "
        "fp32 [3, N] local max, sum-exp, target logit");
  m.def("ce_shard_combine", &ce_shard_combine,
        "vocab-sharded CE: gathered stats [world, 3, N] -> (loss_rows, "
        "lse2), summed in rank order");
  m.def("ce_shard_bwd", &ce_shard_bwd,
        "vocab-sharded CE: (logits, targets, row_start, lse2, dloss_rows) "
        "-> (dlogits bf16 with the logits' row stride, dbias fp32 [V_r])");
  // ce_shard_bwd tiling: columns per strip, rows per chunk
  m.attr("CE_STRIP_COLS") = CE_STRIP_COLS;
  m.attr("CE_BWD_ROWS") = CE_BWD_ROWS;
  m.def("lstmp_cell_fwd", &lstmp_cell_fwd,
        "LSTMP cell step on bf16 MFMA: (gx_t, h_prev, w_hh, bias, c_prev, "
        "c_out, hc_out, gates_out); writes the three outputs");
  m.def("lstmp_cell_bwd", &lstmp_cell_bwd,
        "LSTMP cell step backward: (dh_t, w_hr, gates, c_t, c_prev, dc_next "
        "or None, dgates_out, dc_prev_out); writes the two outputs");
  // lstmp tiling: hidden units / batch rows per workgroup, largest P
  m.attr("LSTMP_TILE_H") = LSTMP_TILE_H;
  m.attr("LSTMP_TILE_B") = LSTMP_TILE_B;
  m.attr("LSTMP_MAX_P") = LSTMP_MAX_P;
  m.def("ssm_prep", &ssm_prep,
        "sampled softmax: (table, bias or None, sampled, targets, logq_samp, "
        "logq_true) -> (Wg [S_pad, P] bf16, Wt [N, P] bf16, off, off0)");
  m.def("ssm_fwd", &ssm_fwd,
        "sampled softmax forward on bf16 MFMA: (h, Wg, Wt, off, off0, "
        "sampled, targets) -> (loss [N], lse2 [N], z0 [N])");
  m.def("ssm_bwd", &ssm_bwd,
        "sampled softmax backward: (h, Wg, off, sampled, targets, lse2, z0, "
        "g) -> (dz [N, S_pad] bf16, dz0 [N], db_samp [S])");
  // ssm tiling: rows per block, columns per tile / per split, largest P
  m.attr("SSM_BM") = SSM_BM;
  m.attr("SSM_BN") = SSM_BN;
  m.attr("SSM_SPLIT_COLS") = SSM_SPLIT_COLS;
  m.attr("SSM_MAX_P") = SSM_MAX_P;
  m.def("lce_compact", &lce_compact,
        "linear + cross-entropy: (h [N, K] bf16, labels [N], ignore_index, "
        "M_cap) -> (Hc [M_cap, K] bf16, rows, tgt, count [1] on the device)");
  m.def("lce_fwd", &lce_fwd,
        "linear + cross-entropy forward on bf16 MFMA: (Hc, weight, bias or "
        "None, rows, tgt, count, N) -> (loss [N], (sum, mean) [2], lse2 "
        "[M_cap])");
  m.def("lce_bwd", &lce_bwd,
        "linear + cross-entropy backward: (Hc, weight, bias or None, rows, "
        "tgt, count, lse2, g_rows [N] or None, g_mean [1] or None) -> (dz "
        "[M_cap, V_ld] bf16, db [V] or None)");
  // lce tiling: vocabulary columns per split
  m.attr("LCE_SPLIT_COLS") = LCE_SPLIT_COLS;
  m.def("neumf_fwd", &neumf_fwd,
        "fused NeuMF forward on fp32 MFMA: (users, items, [mf_user, mf_item, "
        "mlp_user, mlp_item], MLP weights, MLP biases, head weight, head "
        "bias, labels or None, weight or None, save_acts) -> (logits [B], "
        "loss_rows [B], acts [B, sum N_l])");
  m.def("neumf_bwd", &neumf_bwd,
        "fused NeuMF backward: (the forward's operands up to the head bias, "
        "logits, acts, labels or None, weight or None, g_logits or None, "
        "g_loss or None) -> (d_mf_user, d_mf_item, d_mlp_user, d_mlp_item "
        "rows [B, D], dense gradients [P])");
  // neumf limits and tiling: layers, widest layer, samples per block
  m.attr("NEUMF_MAX_LAYERS") = NEUMF_MAX_LAYERS;
  m.attr("NEUMF_MAX_WIDTH") = NEUMF_MAX_WIDTH;
  m.attr("NEUMF_TILE") = NEUMF_TILE;
  m.def("col_sum", &col_sum, "bf16 [N,H] column sum -> fp32 [H]");
  m.def("ln_fwd", &ln_fwd,
        "fused bf16 LayerNorm(+residual) forward -> y, u, mean, rstd");
  m.def("ln_bwd", &ln_bwd, "fused bf16 LayerNorm backward -> dx, dgamma, "
        "dbeta");
  m.def("ln_drop_fwd", &ln_drop_fwd,
        "fused dropout + residual + bf16 LayerNorm forward, "
        "y = LN(dropout_p(x) + res) with the hash mask of seed "
        "-> y, u, mean, rstd",
        py::arg("x"), py::arg("res"), py::arg("gamma"), py::arg("beta"),
        py::arg("eps"), py::arg("p"), py::arg("seed"));
  m.def("ln_drop_bwd", &ln_drop_bwd,
        "one-pass backward of ln_drop_fwd (mask regenerated from seed) "
        "-> dx, dres, dgamma, dbeta",
        py::arg("dy"), py::arg("u"), py::arg("gamma"), py::arg("mean"),
        py::arg("rstd"), py::arg("p"), py::arg("seed"));
  m.def("attn_dropmask", &attn_dropmask,
        "materialize the hash dropout keep-mask (testing)");
  m.def("attn_fwd", &attn_fwd,
        "fused MFMA attention forward (bf16, D=64; optional additive key "
        "mask + hash dropout) — 4-wave LDS-tiled",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("scale"),
        py::arg("mask") = py::none(), py::arg("p_drop") = 0.0,
        py::arg("seed") = 0);
  m.def("attn_fwd_split", &attn_fwd_split,
        "split-KV MFMA attention forward: partial-softmax kernel over "
        "kv_splits key ranges + combine (no dropout)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("scale"),
        py::arg("mask") = py::none(), py::arg("kv_splits") = 1,
        py::arg("p_drop") = 0.0);
  m.attr("ATTN_MAX_SPLITS") = (int)ATTN_MAX_SPLITS;
  m.def("attn_bwd", &attn_bwd,
        "fused MFMA attention backward (GPU-validated) -> dq, dk, dv",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
        py::arg("dout"), py::arg("scale"), py::arg("mask") = py::none(),
        py::arg("p_drop") = 0.0, py::arg("seed") = 0);
}
