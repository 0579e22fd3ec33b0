// vescale_amd C++/HIP extension — single TU: kernels + torch bindings.
//
// Built in-tree for gfx950 only (no multi-backend dispatch, no CUDA shims).
//
// Every binding reads: Binding b(..) (device guard), scalar rules, b.arg(..)
// for EACH tensor, allocate, return early when there is no work, b.launch(..).
// Bindings never copy: callers pass contiguous tensors.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <c10/cuda/CUDAException.h>
#include <c10/cuda/CUDAGuard.h>

#include "rmsnorm.hip"
#include "rope.hip"
#include "rope_qkv.hip"
#include "swiglu.hip"
#include "adamw.hip"
#include "cross_entropy.hip"
#include "philox_random.hip"
#include "gemm.hip"
#include "gemm8.hip"
#include "attention_fwd.hip"
#include "attention_bwd2.hip"
#include "attention_gen.hip"

#include <climits>
#include <sstream>
#include <vector>

namespace {

// ------------------------------ host helpers ------------------------------
constexpr auto BF16 = at::kBFloat16;
constexpr auto F32 = at::kFloat;
constexpr auto I64 = at::kLong;
constexpr auto I32 = at::kInt;
using OptTensor = c10::optional<at::Tensor>;

// typed pointers (bf16 travels as unsigned short); an absent optional is null
inline const unsigned short* bf16(const at::Tensor& t) {
  return reinterpret_cast<const unsigned short*>(t.const_data_ptr());
}
inline unsigned short* bf16_mut(const at::Tensor& t) {
  return reinterpret_cast<unsigned short*>(t.data_ptr());
}
inline const unsigned short* bf16(const OptTensor& t) {
  return t.has_value() ? bf16(*t) : nullptr;
}
inline float* f32(const OptTensor& t) {
  return t.has_value() ? t->data_ptr<float>() : nullptr;
}

// One or two accepted dtypes of an argument.
struct Dtypes {
  at::ScalarType a, b;
  Dtypes(at::ScalarType a) : a(a), b(a) {}
  Dtypes(at::ScalarType a, at::ScalarType b) : a(a), b(b) {}
};

// Expected sizes of an argument (-1: any extent), only its numel, or nothing.
struct Shape {
  at::DimVector sizes;
  int64_t numel = -1;
  bool any = true;
  Shape() {}
  Shape(at::IntArrayRef s) : sizes(s.begin(), s.end()), any(false) {}
  Shape(std::initializer_list<int64_t> s) : sizes(s), any(false) {}
  static Shape of_numel(int64_t n) { Shape s; s.numel = n; return s; }
  bool matches(const at::Tensor& t) const {
    if (any) return numel < 0 || t.numel() == numel;
    if (t.dim() != (int64_t)sizes.size()) return false;
    for (int64_t i = 0; i < t.dim(); ++i)
      if (sizes[i] >= 0 && t.size(i) != sizes[i]) return false;
    return true;
  }
};

// Per-call context: the binding's name, the device of its first tensor and a
// guard on that device, so allocations and the current stream belong to it.
// arg() holds every tensor to that device and launch() holds that device to
// be a GPU, so a call made of CPU tensors still reports a malformed argument
// first and never reaches a kernel.
class Binding {
 public:
  Binding(const char* fn, const char* first_name, const at::Tensor& first)
      : fn(fn), first_name_(first_name), dev_(first.device()) {
    if (first.is_cuda()) guard_.set_device(dev_);
  }

  // The one argument check: device, dtype, contiguity and shape; the
  // message states every fact at once.
  void arg(const char* name, const at::Tensor& t, Dtypes dt, const Shape& shape = {}) const {
    if (t.device() == dev_ && t.is_contiguous() &&
        (t.scalar_type() == dt.a || t.scalar_type() == dt.b) && shape.matches(t))
      return;
    std::ostringstream want;
    want << "device=" << dev_ << (dev_.is_cuda() ? "" : " (must be a GPU)")
         << " dtype=" << c10::toString(dt.a);
    if (dt.b != dt.a) want << "|" << c10::toString(dt.b);
    if (!shape.any) want << " sizes=" << at::IntArrayRef(shape.sizes);
    if (shape.numel >= 0) want << " numel=" << shape.numel;
    TORCH_CHECK(false, fn, ": argument '", name, "' expected ", want.str(),
                " contiguous=true; got device=", t.device(), " dtype=",
                c10::toString(t.scalar_type()), " sizes=", t.sizes(), " numel=",
                t.numel(), " contiguous=", t.is_contiguous() ? "true" : "false");
  }
  void arg(const char* name, const OptTensor& t, Dtypes dt, const Shape& shape = {}) const {
    if (t.has_value()) arg(name, *t, dt, shape);
  }

  // Last dimension of a [..., n] argument; n must be a positive multiple of mult.
  int64_t last_dim(const char* what, const at::Tensor& t, int mult) const {
    int64_t n = t.dim() >= 1 ? t.size(-1) : 0;
    TORCH_CHECK(n > 0 && n % mult == 0, fn, ": ", what, " = ", n,
                " must be a positive multiple of ", mult);
    return n;
  }

  // The rope table must cover positions [pos_offset, pos_offset + S).
  void rope_span(const at::Tensor& table, int64_t pos_offset, int64_t S, int64_t D) const {
    TORCH_CHECK(D > 0 && D % 2 == 0, fn, ": head dim D = ", D, " must be even");
    TORCH_CHECK(pos_offset >= 0, fn, ": pos_offset = ", pos_offset, " must be >= 0");
    TORCH_CHECK(table.dim() == 3 && pos_offset + S <= table.size(0), fn,
                ": pos_offset + S = ", pos_offset + S, " is past the table, sizes=",
                table.sizes());
  }

  // The only launch site: on the current stream, never a zero-size grid,
  // launch error checked.  Host-only (no sync, no allocation, no device
  // query), so it is safe under graph capture.
  template <typename... KArgs, typename... Args>
  void launch(void (*kernel)(KArgs...), dim3 grid, dim3 block, Args&&... args) const {
    TORCH_CHECK(dev_.is_cuda(), fn, ": argument '", first_name_,
                "' expected device=a GPU; got device=", dev_);
    TORCH_CHECK(grid.x > 0 && grid.y > 0 && grid.z > 0, fn, ": zero grid dimension (",
                grid.x, ",", grid.y, ",", grid.z, "); return before launching when there is no work");
    hipLaunchKernelGGL(kernel, grid, block, 0,
                       (hipStream_t)at::cuda::getCurrentCUDAStream().stream(),
                       std::forward<Args>(args)...);
    C10_CUDA_KERNEL_LAUNCH_CHECK();
  }

  const char* const fn;

 private:
  const char* first_name_;
  c10::Device dev_;
  at::cuda::OptionalCUDAGuard guard_;
};

}  // namespace

#include "probes.hip"

namespace {

// ------------------------------ RMSNorm ------------------------------
std::vector<at::Tensor> rmsnorm_fwd(at::Tensor x, at::Tensor w, double eps) {
  Binding b("rmsnorm_fwd", "x", x);
  int hidden = (int)b.last_dim("hidden (x.size(-1))", x, 8);
  b.arg("x", x, BF16);
  b.arg("w", w, BF16, {hidden});
  int64_t rows = x.numel() / hidden;
  auto out = at::empty_like(x);
  auto rrms = at::empty({rows}, x.options().dtype(F32));
  if (rows == 0) return {out, rrms};
  b.launch(rmsnorm_fwd_bf16, (int)std::min<int64_t>(rows, 2048), 256, bf16(x), bf16(w),
           bf16_mut(out), rrms.data_ptr<float>(), rows, hidden, (float)eps);
  return {out, rrms};
}

std::vector<at::Tensor> rmsnorm_bwd(at::Tensor dy, at::Tensor x, at::Tensor w,
                                    at::Tensor rrms, OptTensor dres) {
  Binding b("rmsnorm_bwd", "dy", dy);
  int hidden = (int)b.last_dim("hidden (dy.size(-1))", dy, 8);
  TORCH_CHECK(hidden <= 8192, "rmsnorm_bwd supports hidden <= 8192, got ", hidden);
  int64_t rows = dy.numel() / hidden;
  b.arg("dy", dy, BF16);
  b.arg("x", x, BF16, dy.sizes());
  b.arg("w", w, BF16, {hidden});
  b.arg("rrms", rrms, F32, {rows});
  b.arg("dres", dres, BF16, dy.sizes());
  auto dx = at::empty_like(x);
  if (rows == 0) return {dx, at::zeros({hidden}, x.options().dtype(F32))};
  int grid = (int)std::min<int64_t>(rows, 1024);
  // one dw row per block, summed below in a fixed order (deterministic)
  auto dw_part = at::empty({grid, hidden}, x.options().dtype(F32));
  // the instantiation with just enough 8-element chunks per thread
  decltype(&rmsnorm_bwd_bf16) kerns[] = {rmsnorm_bwd_it1_bf16, rmsnorm_bwd_it2_bf16,
                                         rmsnorm_bwd_it3_bf16, rmsnorm_bwd_bf16};
  b.launch(kerns[(hidden - 1) / 2048], grid, 256, bf16(dy), bf16(x), bf16(w),
           rrms.data_ptr<float>(), bf16(dres), bf16_mut(dx), dw_part.data_ptr<float>(),
           rows, hidden);
  return {dx, dw_part.sum(0)};
}

std::vector<at::Tensor> rmsnorm_res_fwd(at::Tensor x, OptTensor res, at::Tensor w,
                                        double eps) {
  // fused residual add + rmsnorm: returns {norm_out, res_new, rrms}
  Binding b("rmsnorm_res_fwd", "x", x);
  int hidden = (int)b.last_dim("hidden (x.size(-1))", x, 8);
  b.arg("x", x, BF16);
  b.arg("res", res, BF16, x.sizes());
  b.arg("w", w, BF16, {hidden});
  int64_t rows = x.numel() / hidden;
  auto out = at::empty_like(x);
  auto res_out = at::empty_like(x);
  auto rrms = at::empty({rows}, x.options().dtype(F32));
  if (rows == 0) return {out, res_out, rrms};
  b.launch(rmsnorm_res_fwd_bf16, (int)std::min<int64_t>(rows, 2048), 256, bf16(x),
           bf16(res), bf16(w), bf16_mut(out), bf16_mut(res_out), rrms.data_ptr<float>(),
           rows, hidden, (float)eps);
  return {out, res_out, rrms};
}

// ------------------------------ RoPE ------------------------------
at::Tensor rope(at::Tensor x, at::Tensor table, int64_t pos_offset, bool backward,
                bool inplace) {
  // x: [B, S, H, D] bf16, table: [S_max, D/2, 2] f32
  Binding b("rope", "x", x);
  TORCH_CHECK(x.dim() == 4, "rope: x must be [B,S,H,D], got sizes=", x.sizes());
  int B = (int)x.size(0), S = (int)x.size(1), H = (int)x.size(2), D = (int)x.size(3);
  b.rope_span(table, pos_offset, S, D);
  b.arg("x", x, BF16);
  b.arg("table", table, F32, {-1, D / 2, 2});
  auto out = inplace ? x : at::empty_like(x);
  int64_t n_tokens = (int64_t)B * S * H;
  int64_t pairs = n_tokens * (D / 2);
  b.launch(rope_fwd_bf16, grid_for(pairs / 2, 256), 256, bf16(x), bf16_mut(out),
           table.data_ptr<float>(), n_tokens, H, S, D, (int)pos_offset,
           backward ? 1 : 0);
  return out;
}

// Scalar rules shared by rope_qkv_fwd / rope_qkv_bwd; returns the number of
// (token, head, pair) work items.
int64_t rope_qkv_check(const Binding& b, const at::Tensor& table, int64_t B, int64_t S,
                       int64_t Hq, int64_t Hkv, int64_t D, int64_t pos_offset) {
  TORCH_CHECK(B >= 0 && S >= 0 && Hq >= 0 && Hkv >= 0 && D <= INT_MAX &&
                  S <= INT_MAX && Hq <= INT_MAX && Hkv <= INT_MAX,
              b.fn, ": B, S, Hq, Hkv must be >= 0 and fit int");
  b.rope_span(table, pos_offset, S, D);
  return B * S * (Hq + 2 * Hkv) * (D / 2);
}

// The 16-byte kernels take D % 16 == 0 with at most 64 units of 16 elements
// per head (one wave covers a head) and 16-byte aligned tensors; every other
// call runs the scalar kernels.
bool rope_qkv_v8(int64_t D, std::initializer_list<const at::Tensor*> ts) {
  if (D % 16 != 0 || D / 16 > 64) return false;
  for (const at::Tensor* t : ts)
    if (reinterpret_cast<uintptr_t>(t->const_data_ptr()) % 16 != 0) return false;
  return true;
}
// one wave per token, 4 tokens per block pass
int rope_qkv_v8_grid(int64_t tokens) { return grid_for(tokens, 4, 1 << 16); }

std::vector<at::Tensor> rope_qkv_fwd(at::Tensor qkv, at::Tensor table, int64_t B,
                                     int64_t S, int64_t Hq, int64_t Hkv, int64_t D,
                                     int64_t pos_offset) {
  Binding b("rope_qkv_fwd", "qkv", qkv);
  int64_t total = rope_qkv_check(b, table, B, S, Hq, Hkv, D, pos_offset);
  b.arg("qkv", qkv, BF16, Shape::of_numel(total * 2));
  b.arg("table", table, F32, {-1, D / 2, 2});
  auto opt = qkv.options();
  auto q = at::empty({B, Hq, S, D}, opt);
  auto k = at::empty({B, Hkv, S, D}, opt);
  auto v = at::empty({B, Hkv, S, D}, opt);
  if (total == 0) return {q, k, v};
  const bool v8 = rope_qkv_v8(D, {&qkv, &q, &k, &v, &table});
  b.launch(v8 ? rope_qkv_fwd_v8_bf16 : rope_qkv_fwd_bf16,
           v8 ? rope_qkv_v8_grid(B * S) : grid_for(total, 256), 256, bf16(qkv), bf16_mut(q),
           bf16_mut(k), bf16_mut(v), table.data_ptr<float>(), B * S, (int)S, (int)Hq,
           (int)Hkv, (int)D, (int)pos_offset);
  return {q, k, v};
}

at::Tensor rope_qkv_bwd(at::Tensor dq, at::Tensor dk, at::Tensor dv, at::Tensor table,
                        int64_t B, int64_t S, int64_t Hq, int64_t Hkv, int64_t D,
                        int64_t pos_offset) {
  Binding b("rope_qkv_bwd", "dq", dq);
  int64_t total = rope_qkv_check(b, table, B, S, Hq, Hkv, D, pos_offset);
  b.arg("dq", dq, BF16, {B, Hq, S, D});
  b.arg("dk", dk, BF16, {B, Hkv, S, D});
  b.arg("dv", dv, BF16, {B, Hkv, S, D});
  b.arg("table", table, F32, {-1, D / 2, 2});
  auto dqkv = at::empty({B, S, (Hq + 2 * Hkv) * D}, dq.options());
  if (total == 0) return dqkv;
  const bool v8 = rope_qkv_v8(D, {&dq, &dk, &dv, &dqkv, &table});
  b.launch(v8 ? rope_qkv_bwd_v8_bf16 : rope_qkv_bwd_bf16,
           v8 ? rope_qkv_v8_grid(B * S) : grid_for(total, 256), 256, bf16(dq), bf16(dk),
           bf16(dv), bf16_mut(dqkv), table.data_ptr<float>(), B * S, (int)S, (int)Hq,
           (int)Hkv, (int)D, (int)pos_offset);
  return dqkv;
}

// ------------------------------ SwiGLU ------------------------------
at::Tensor swiglu_fwd(at::Tensor gate, at::Tensor up) {
  Binding b("swiglu_fwd", "gate", gate);
  b.arg("gate", gate, BF16);
  b.arg("up", up, BF16, gate.sizes());
  auto out = at::empty_like(gate);
  int64_t n = gate.numel();
  b.launch(swiglu_fwd_bf16, grid_for(n / 8, 256), 256, bf16(gate), bf16(up),
           bf16_mut(out), n);
  return out;
}

std::vector<at::Tensor> swiglu_bwd(at::Tensor dy, at::Tensor gate, at::Tensor up) {
  Binding b("swiglu_bwd", "dy", dy);
  b.arg("dy", dy, BF16);
  b.arg("gate", gate, BF16, dy.sizes());
  b.arg("up", up, BF16, dy.sizes());
  auto dgate = at::empty_like(gate);
  auto dup = at::empty_like(up);
  int64_t n = gate.numel();
  b.launch(swiglu_bwd_bf16, grid_for(n / 8, 256), 256, bf16(dy), bf16(gate), bf16(up),
           bf16_mut(dgate), bf16_mut(dup), n);
  return {dgate, dup};
}

at::Tensor swiglu_packed_fwd(at::Tensor gu) {
  Binding b("swiglu_packed_fwd", "gu", gu);
  int F = (int)b.last_dim("packed ffn dim F2 (gu.size(-1))", gu, 16) / 2;
  b.arg("gu", gu, BF16);
  int64_t rows = gu.numel() / (2 * F);
  auto sizes = gu.sizes().vec();
  sizes.back() = F;
  auto out = at::empty(sizes, gu.options());
  b.launch(swiglu_packed_fwd_bf16, grid_for(rows * (F / 8), 256), 256, bf16(gu),
           bf16_mut(out), rows, F);
  return out;
}

at::Tensor swiglu_packed_bwd(at::Tensor dy, at::Tensor gu) {
  Binding b("swiglu_packed_bwd", "dy", dy);
  int F = (int)b.last_dim("packed ffn dim F2 (gu.size(-1))", gu, 16) / 2;
  auto sizes = gu.sizes().vec();
  sizes.back() = F;
  b.arg("dy", dy, BF16, at::IntArrayRef(sizes));
  b.arg("gu", gu, BF16);
  int64_t rows = gu.numel() / (2 * F);
  auto dgu = at::empty_like(gu);
  b.launch(swiglu_packed_bwd_bf16, grid_for(rows * (F / 8), 256), 256, bf16(dy),
           bf16(gu), bf16_mut(dgu), rows, F);
  return dgu;
}

// ------------------------------ Cross entropy ------------------------------
// Target VALUES are not read here (that would need a device sync): every
// target inside [0, vocab) or equal to ignore_index is the caller's duty.
//
// vocab_total == -1 (the default) is the dense pair.  vocab_total >= 0 is the
// vocab-parallel pair: logits holds columns [vocab_start, vocab_start + n) of
// a vocab_total-class row and targets are global ids of ANY value (the
// kernels compare, they never index with an unchecked target).

// The column range of a vocab-parallel call must lie inside the vocabulary.
void ce_vp_check(const Binding& b, int64_t n, int64_t vocab_start, int64_t vocab_total) {
  TORCH_CHECK(vocab_total >= -1, b.fn, ": vocab_total = ", vocab_total,
              " must be >= 0, or -1 for the dense kernel");
  TORCH_CHECK(vocab_start >= 0, b.fn, ": vocab_start = ", vocab_start, " must be >= 0");
  TORCH_CHECK(vocab_total == -1 ? vocab_start == 0 : vocab_start <= vocab_total - n, b.fn,
              ": vocab_start + n = ", vocab_start, " + ", n,
              " is past vocab_total = ", vocab_total);
}

// dense: {loss, lse}; vocab-parallel: {picked, lse_local}
std::vector<at::Tensor> ce_fwd(at::Tensor logits, at::Tensor target,
                               int64_t ignore_index, int64_t vocab_start,
                               int64_t vocab_total) {
  Binding b("ce_fwd", "logits", logits);
  int vocab = (int)b.last_dim("vocab (logits.size(-1))", logits, 8);
  ce_vp_check(b, vocab, vocab_start, vocab_total);
  int64_t rows = logits.numel() / vocab;
  b.arg("logits", logits, BF16);
  b.arg("target", target, I64, Shape::of_numel(rows));
  auto loss = at::empty({rows}, logits.options().dtype(F32));
  auto lse = at::empty({rows}, logits.options().dtype(F32));
  if (rows == 0) return {loss, lse};
  int grid = (int)std::min<int64_t>(rows, 2048);
  if (vocab_total < 0)
    b.launch(ce_fwd_bf16, grid, 256, bf16(logits), target.data_ptr<int64_t>(),
             loss.data_ptr<float>(), lse.data_ptr<float>(), rows, vocab, ignore_index);
  else
    b.launch(ce_vp_fwd_bf16, grid, 256, bf16(logits), target.data_ptr<int64_t>(),
             loss.data_ptr<float>(), lse.data_ptr<float>(), rows, vocab, vocab_start,
             ignore_index);
  return {loss, lse};
}

// lse: the row's log-sum-exp over the WHOLE vocabulary in either form
at::Tensor ce_bwd(at::Tensor logits, at::Tensor target, at::Tensor lse,
                  at::Tensor dloss, int64_t ignore_index, bool inplace,
                  int64_t vocab_start, int64_t vocab_total) {
  Binding b("ce_bwd", "logits", logits);
  int vocab = (int)b.last_dim("vocab (logits.size(-1))", logits, 8);
  ce_vp_check(b, vocab, vocab_start, vocab_total);
  int64_t rows = logits.numel() / vocab;
  b.arg("logits", logits, BF16);
  b.arg("target", target, I64, Shape::of_numel(rows));
  b.arg("lse", lse, F32, {rows});
  b.arg("dloss", dloss, F32, {rows});
  auto dlogits = inplace ? logits : at::empty_like(logits);
  if (rows == 0) return dlogits;
  int grid = (int)std::min<int64_t>(rows, 2048);
  if (vocab_total < 0)
    b.launch(ce_bwd_bf16, grid, 256, bf16(logits), bf16_mut(dlogits),
             target.data_ptr<int64_t>(), lse.data_ptr<float>(), dloss.data_ptr<float>(),
             rows, vocab, ignore_index);
  else
    b.launch(ce_vp_bwd_bf16, grid, 256, bf16(logits), bf16_mut(dlogits),
             target.data_ptr<int64_t>(), lse.data_ptr<float>(), dloss.data_ptr<float>(),
             rows, vocab, vocab_start, ignore_index);
  return dlogits;
}

// ------------------------------ AdamW ------------------------------
void adamw_step(at::Tensor param, OptTensor master, at::Tensor grad, at::Tensor m,
                at::Tensor v, double lr, double beta1, double beta2, double eps,
                double weight_decay, int64_t step, double grad_scale,
                OptTensor clip_scale) {
  Binding b("adamw_step", "param", param);
  TORCH_CHECK(step >= 1, "adamw_step: step = ", step, " must be >= 1");
  int64_t n = param.numel();
  b.arg("param", param, BF16);
  b.arg("master", master, F32, Shape::of_numel(n));
  b.arg("grad", grad, {BF16, F32}, Shape::of_numel(n));
  b.arg("m", m, F32, Shape::of_numel(n));
  b.arg("v", v, F32, Shape::of_numel(n));
  b.arg("clip_scale", clip_scale, F32);
  TORCH_CHECK(!clip_scale.has_value() || clip_scale->numel() >= 1,
              "adamw_step: argument 'clip_scale' needs at least one element");
  float bc1 = 1.f - powf((float)beta1, (float)step);
  float bc2 = 1.f - powf((float)beta2, (float)step);
  bool gbf = grad.scalar_type() == BF16;
  b.launch(adamw_flat_bf16, grid_for(n / 8, 256), 256, bf16_mut(param), f32(master),
           gbf ? bf16(grad) : nullptr, gbf ? nullptr : grad.data_ptr<float>(),
           m.data_ptr<float>(), v.data_ptr<float>(), n, (float)lr, (float)beta1,
           (float)beta2, (float)eps, (float)weight_decay, bc1, bc2, (float)grad_scale,
           f32(clip_scale));
}

at::Tensor l2norm_sq(at::Tensor x) {
  Binding b("l2norm_sq", "x", x);
  b.arg("x", x, {BF16, F32});
  int64_t n = x.numel();
  if (n == 0) return at::zeros({1}, x.options().dtype(F32));
  int grid = grid_for(n / 8, 256);
  auto part = at::empty({grid}, x.options().dtype(F32));
  bool xbf = x.scalar_type() == BF16;
  b.launch(l2norm_sq_flat, grid, 256, xbf ? bf16(x) : nullptr,
           xbf ? nullptr : x.data_ptr<float>(), part.data_ptr<float>(), n);
  return part.sum(0, /*keepdim=*/true);
}

void scale_(at::Tensor x, OptTensor scale_t, double scale_c) {
  Binding b("scale_", "x", x);
  b.arg("x", x, {BF16, F32});
  b.arg("scale_t", scale_t, F32);
  TORCH_CHECK(!scale_t.has_value() || scale_t->numel() >= 1,
              "scale_: argument 'scale_t' needs at least one element");
  int64_t n = x.numel();
  if (n == 0) return;
  bool xbf = x.scalar_type() == BF16;
  b.launch(scale_flat, grid_for(n / 8, 256), 256, xbf ? bf16_mut(x) : nullptr,
           xbf ? nullptr : x.data_ptr<float>(), f32(scale_t), (float)scale_c, n);
}

// ------------------------------ MFMA GEMM ------------------------------
// C[M,N] = a[M,K] @ b[N,K]^T: operand checks shared by gemm_tn / gemm_tn8.
void gemm_check(const Binding& b, const at::Tensor& a, const at::Tensor& bm, int BM,
                int BN, int BK) {
  TORCH_CHECK(a.dim() == 2 && bm.dim() == 2, b.fn, ": a and b must be 2-D, got a sizes=",
              a.sizes(), " b sizes=", bm.sizes());
  int64_t M = a.size(0), K = a.size(1), N = bm.size(0);
  TORCH_CHECK(M >= 1 && N >= 1 && K >= 1 && M <= INT_MAX && N <= INT_MAX && K <= INT_MAX,
              b.fn, ": M, N, K must be >= 1 and fit int");
  TORCH_CHECK(M % BM == 0 && N % BN == 0 && K % BK == 0, b.fn,
              " tile divisibility violated: requires M % ", BM, " == 0, N % ", BN,
              " == 0 and K % ", BK, " == 0");
  b.arg("a", a, BF16);
  b.arg("b", bm, BF16, {N, K});
}

at::Tensor gemm_tn(at::Tensor a, at::Tensor b, int64_t variant) {
  Binding bd("gemm_tn", "a", a);
  TORCH_CHECK(variant >= 0 && variant <= 4, "gemm_tn: variant = ", variant,
              " must be in 0..4");
  int BM = variant == 1 ? 128 : (variant == 3 ? 128 : (variant == 4 ? 512 : 256));
  int BN = variant == 3 ? 128 : 256;
  int BK = variant == 1 ? 64 : 32;
  int threads = variant == 3 ? 256 : (variant == 4 ? 1024 : 512);
  gemm_check(bd, a, b, BM, BN, BK);
  int64_t M = a.size(0), K = a.size(1), N = b.size(0);
  auto c = at::empty({M, N}, a.options());
  decltype(&gemm_tn_bf16_v0) kerns[] = {gemm_tn_bf16_v0, gemm_tn_bf16_v1, gemm_tn_bf16_v2,
                                        gemm_tn_bf16_v3, gemm_tn_bf16_v4};
  bd.launch(kerns[variant], (int)((M / BM) * (N / BN)), threads, bf16(a), bf16(b),
            bf16_mut(c), (int)M, (int)N, (int)K);
  return c;
}

at::Tensor gemm_tn8(at::Tensor a, at::Tensor b, int64_t mode) {
  // via the 8-phase 256x256 template (gemm8.hip)
  Binding bd("gemm_tn8", "a", a);
  TORCH_CHECK(mode >= 0 && mode <= 8, "gemm_tn8: mode = ", mode, " must be in 0..8");
  gemm_check(bd, a, b, G8_BM, G8_BN, G8_BK);
  int64_t M = a.size(0), K = a.size(1), N = b.size(0);
  TORCH_CHECK(mode != 5 || (K / 64) % 2 == 0, "mode 5 needs K % 128 == 0");
  TORCH_CHECK((mode != 7 && mode != 8) || ((K / 64) % 2 == 0 && K / 64 >= 4),
              "modes 7/8 need an even K/64 >= 4");
  auto c = at::empty({M, N}, a.options());
  decltype(&gemm8_tn_bf16) kerns[] = {  // indexed by mode
      gemm8_tn_bf16,        gemm8_tn_bf16_lockstep, gemm8_tn_bf16_rot,
      gemm8_tn_bf16_rot3,   gemm8_tn_bf16_rot3np,   gemm8_tn_bf16_rot3u2,
      gemm8_tn_bf16_rot3ra, gemm8_tn_bf16_rot8,     gemm8_tn_bf16_rot9};
  bd.launch(kerns[mode], dim3((unsigned)(M / 256), (unsigned)(N / 256), 1), G8_THREADS,
            bf16(a), bf16(b), bf16_mut(c), (int)M, (int)N, (int)K);
  return c;
}

// ------------------------------ tuned flash attention (causal, D=128) ------
struct FaShape { int B, Hq, Hkv, S; };

// q: [B,Hq,S,128]; k,v: [B,Hkv,S,128]; lse: [B,Hq,S] f32; S % tile == 0.
// o,dout: [B,Hq,S,128], or with bshd [B,S,Hq,128].  The forward bindings pass
// no o/dout/lse.
FaShape fa_check(const Binding& b, int tile, const at::Tensor& q, const at::Tensor& k,
                 const at::Tensor& v, const OptTensor& o = {},
                 const OptTensor& dout = {}, const OptTensor& lse = {}, bool bshd = false) {
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4, b.fn, ": q, k must be [B,H,S,128], got q sizes=",
              q.sizes(), " k sizes=", k.sizes());
  int64_t B = q.size(0), Hq = q.size(1), S = q.size(2), Hkv = k.size(1);
  TORCH_CHECK(S >= 1 && S % tile == 0 && S <= INT_MAX, b.fn, ": seq = ", S,
              " must be a positive multiple of ", tile);
  TORCH_CHECK(B >= 1 && Hkv >= 1 && Hq >= 1 && Hq % Hkv == 0, b.fn, ": B = ", B,
              " must be >= 1 and Hq = ", Hq, " a positive multiple of Hkv = ", Hkv);
  b.arg("q", q, BF16, {B, Hq, S, FF_D});
  b.arg("k", k, BF16, {B, Hkv, S, FF_D});
  b.arg("v", v, BF16, {B, Hkv, S, FF_D});
  // the [B,S,Hq,D] kernels index rows and a 256-row tile's elements in int
  TORCH_CHECK(!bshd || (B * Hq * S <= INT_MAX && Hq * FF_D * 256 <= INT_MAX), b.fn,
              ": B * Hq * S and Hq * 32768 must fit int in the [B,S,Hq,D] layout");
  const Shape oshape = bshd ? Shape{B, S, Hq, FF_D} : Shape{B, Hq, S, FF_D};
  b.arg("o", o, BF16, oshape);
  b.arg("dout", dout, BF16, oshape);
  b.arg("lse", lse, F32, {B, Hq, S});
  return {(int)B, (int)Hq, (int)Hkv, (int)S};
}
static_assert(FB_D == FF_D, "tuned attention kernels share D");

// out_bshd: o is allocated and written as [B,S,Hq,D]; lse stays [B,Hq,S]
std::vector<at::Tensor> fa_fwd_impl(const Binding& b, int64_t mode, at::Tensor q,
                                    at::Tensor k, at::Tensor v, double scale,
                                    bool out_bshd) {
  FaShape s = fa_check(b, FF_QTILE, q, k, v);
  TORCH_CHECK(!out_bshd || (int64_t)s.Hq * FF_D <= INT_MAX, b.fn,
              ": Hq * 128 must fit int in the [B,S,Hq,D] layout");
  auto out = out_bshd ? at::empty({s.B, s.S, s.Hq, FF_D}, q.options()) : at::empty_like(q);
  auto lse = at::empty({s.B, s.Hq, s.S}, q.options().dtype(F32));
  decltype(&fa_fwd_bf16) kerns[] = {fa_fwd_bf16,     fa_fwd_bf16_ab1, fa_fwd_bf16_ab2,
                                    fa_fwd_bf16_ab3, fa_fwd_bf16_ab4, fa_fwd_bf16_ab5};
  b.launch(kerns[mode], dim3(s.S / FF_QTILE, s.Hq, s.B), FF_THREADS, bf16(q), bf16(k), bf16(v),
           bf16_mut(out), lse.data_ptr<float>(), s.B, s.Hq, s.Hkv, s.S, (float)scale,
           out_bshd ? 1 : 0);
  return {out, lse};
}

std::vector<at::Tensor> fa_fwd(at::Tensor q, at::Tensor k, at::Tensor v, double scale,
                               bool out_bshd) {
  return fa_fwd_impl(Binding("fa_fwd", "q", q), 0, q, k, v, scale, out_bshd);
}

std::vector<at::Tensor> fa_fwd_ablate(at::Tensor q, at::Tensor k, at::Tensor v,
                                      double scale, int64_t mode) {
  // ablation-timing variants of fa_fwd (NOT numerically meaningful for
  // mode != 0); see attention_fwd.hip template MODE docs
  TORCH_CHECK(mode >= 0 && mode <= 5, "fa_fwd_ablate: mode = ", mode,
              " must be in 0..5");
  return fa_fwd_impl(Binding("fa_fwd_ablate", "q", q), mode, q, k, v, scale, false);
}

// delta[b,h,s] = sum_d dout * o for fa_bwd2; bshd: dout and o are [B,S,Hq,D]
at::Tensor fa_bwd_delta(const Binding& b, const FaShape& s, const at::Tensor& dout,
                        const at::Tensor& o, bool bshd = false) {
  auto delta = at::empty({s.B, s.Hq, s.S}, o.options().dtype(F32));
  int64_t rows = (int64_t)s.B * s.Hq * s.S;
  b.launch(fa_bwd_preprocess, grid_for(rows, 1, 4096), 256, bf16(dout), bf16(o),
           delta.data_ptr<float>(), rows, s.Hq, s.S, bshd ? 1 : 0);
  return delta;
}

// [B,Hq,S,D] per-q-head partial -> [B,Hkv,S,D] (identity when Hkv == Hq)
at::Tensor fa_bwd_reduce(const Binding& b, const FaShape& s, const at::Tensor& part) {
  if (s.Hkv == s.Hq) return part;
  auto out = at::empty({s.B, s.Hkv, s.S, FF_D}, part.options());
  int64_t SD = (int64_t)s.S * FF_D;
  b.launch(fa_bwd_reduce_gqa, grid_for((int64_t)s.B * s.Hkv * SD / 8, 256), 256,
           bf16(part), bf16_mut(out), s.B, s.Hq, s.Hkv, SD);
  return out;
}

// ------------------------------ flash-attention backward v2 ---------------
std::vector<at::Tensor> fa_bwd2(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                                at::Tensor dout, at::Tensor lse, double scale,
                                bool fused_dvdk, bool bshd) {
  // 32x32-MFMA backward (attention_bwd2.hip): preprocess + dq + dv + dk
  // (+ GQA reduction); lse ln-domain.  bshd: o and dout are [B,S,Hq,D] (the
  // split kernels only); dq/dk/dv are [B,H,S,D] either way.
  Binding b("fa_bwd2", "q", q);
  TORCH_CHECK(!(bshd && fused_dvdk), "fa_bwd2: the fused dv+dk kernel reads [B,Hq,S,D] ",
              "only: bshd=True needs fused_dvdk=False");
  FaShape s = fa_check(b, FB_TILE, q, k, v, o, dout, lse, bshd);
  // the kernels write -inf into the masked scores BEFORE scaling them
  // (ff_mask): only a positive finite scale keeps them -inf
  TORCH_CHECK(scale > 0 && std::isfinite(scale), b.fn, ": scale = ", scale,
              " must be positive and finite");
  auto delta = fa_bwd_delta(b, s, dout, o, bshd);
  auto dq = at::empty_like(q);
  dim3 grid(s.S / FB_TILE, s.Hq, s.B);
  b.launch(fa2_dq_bf16, grid, FB_THREADS, bf16(q), bf16(k), bf16(v), bf16(dout),
           lse.data_ptr<float>(), delta.data_ptr<float>(), bf16_mut(dq), s.B, s.Hq,
           s.Hkv, s.S, (float)scale, bshd ? 1 : 0);
  auto dv_part = at::empty_like(q);
  auto dk_part = at::empty_like(q);
  if (fused_dvdk) {
    // 4-wave blocks over 128-row kv tiles (see kernel comment): 2x the
    // blocks of the split kernels' 256-row tiles.
    b.launch(fa2_dvdk_bf16, dim3(s.S / FD_TILE, s.Hq, s.B), FD_THREADS, bf16(q),
             bf16(k), bf16(v), bf16(dout), lse.data_ptr<float>(),
             delta.data_ptr<float>(), bf16_mut(dv_part), bf16_mut(dk_part), s.B, s.Hq,
             s.Hkv, s.S, (float)scale);
  } else {
    b.launch(fa2_dv_bf16, grid, FB_THREADS, bf16(q), bf16(k), bf16(dout),
             lse.data_ptr<float>(), bf16_mut(dv_part), s.B, s.Hq, s.Hkv, s.S,
             (float)scale, bshd ? 1 : 0);
    b.launch(fa2_dk_bf16, grid, FB_THREADS, bf16(q), bf16(k), bf16(v), bf16(dout),
             lse.data_ptr<float>(), delta.data_ptr<float>(), bf16_mut(dk_part), s.B,
             s.Hq, s.Hkv, s.S, (float)scale, bshd ? 1 : 0);
  }
  return {dq, fa_bwd_reduce(b, s, dk_part), fa_bwd_reduce(b, s, dv_part)};
}

// ------------------------------ general-shape flash attention --------------
struct FaGenShape { int B, Hq, Hkv, Sq, Sk, D, shift; bool seg; };

FaGenShape fa_gen_check(const Binding& b, const at::Tensor& q, const at::Tensor& k,
                        const at::Tensor& v, bool causal, int64_t shift,
                        const OptTensor& q_seg, const OptTensor& kv_seg) {
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4,
              b.fn, ": q, k, v must be [B, H, S, D]");
  int64_t D = q.size(3);
  TORCH_CHECK(D == 64 || D == 128, b.fn, ": fa_gen supports head_dim 64 and 128");
  TORCH_CHECK(k.size(1) >= 1 && q.size(1) % k.size(1) == 0,
              b.fn, ": Hq must be a multiple of Hkv");
  TORCH_CHECK(q.size(2) >= 1 && k.size(2) >= 1, b.fn, ": Sq and Sk must be >= 1");
  TORCH_CHECK(q.size(0) >= 1 && q.size(0) <= 65535 && q.size(1) <= 65535,
              b.fn, ": B and Hq must be in [1, 65535]");
  TORCH_CHECK(q.size(2) + k.size(2) < (int64_t)1 << 30, b.fn, ": sequence too long");
  TORCH_CHECK(causal || shift == 0, b.fn, ": shift needs causal");
  TORCH_CHECK(q_seg.has_value() == kv_seg.has_value(), b.fn,
              ": q_seg and kv_seg must be given together");
  b.arg("q", q, BF16);
  b.arg("k", k, BF16, {q.size(0), -1, -1, D});  // [B, Hkv, Sk, D]
  b.arg("v", v, BF16, k.sizes());
  b.arg("q_seg", q_seg, I32, {q.size(0), q.size(2)});    // [B, Sq]
  b.arg("kv_seg", kv_seg, I32, {q.size(0), k.size(2)});  // [B, Sk]
  // clamping to [-Sq, Sk] leaves the mask j <= i + shift unchanged
  int64_t sh = std::max<int64_t>(-q.size(2), std::min<int64_t>(k.size(2), shift));
  return {(int)q.size(0), (int)q.size(1), (int)k.size(1), (int)q.size(2),
          (int)k.size(2), (int)D, (int)sh, q_seg.has_value()};
}

// The one place that picks a general kernel's instantiation: head dim, and
// the segment-masked variant when the call carries segment ids.
#define FA_GEN_KERNEL(kernel, D) ((D) == 64 ? kernel<64> : kernel<128>)
#define FA_GEN_KERNEL_SEG(kernel, s)                                        \
  ((s).seg ? ((s).D == 64 ? kernel<64, true> : kernel<128, true>)           \
           : ((s).D == 64 ? kernel<64, false> : kernel<128, false>))

// Segment pre-pass: (min, max) id of every 64-row q and kv tile, the facts
// the kernels skip tile pairs on.  Launched by both bindings (the backward
// re-runs it: nothing crosses the autograd node but the ids themselves).
// Without segment ids there is no launch and the kernels get null pointers.
struct FaGenSeg {
  at::Tensor bounds;
  const int* q = nullptr;
  const int* kv = nullptr;
  const int* tiles = nullptr;
};

FaGenSeg fa_gen_seg(const Binding& b, const FaGenShape& s, const at::Tensor& like,
                    const OptTensor& q_seg, const OptTensor& kv_seg) {
  FaGenSeg g;
  if (!s.seg) return g;
  int tiles = (s.Sq + FG_BLK - 1) / FG_BLK + (s.Sk + FG_BLK - 1) / FG_BLK;
  g.bounds = at::empty({s.B, tiles, 2}, like.options().dtype(I32));
  g.q = q_seg->data_ptr<int>();
  g.kv = kv_seg->data_ptr<int>();
  b.launch(fa_gen_seg_bounds_kernel, dim3(tiles, s.B), FG_BLK, g.q, g.kv,
           g.bounds.data_ptr<int>(), s.Sq, s.Sk);
  g.tiles = g.bounds.data_ptr<int>();
  return g;
}

std::vector<at::Tensor> fa_gen_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                   double scale, bool causal, int64_t shift,
                                   OptTensor q_seg, OptTensor kv_seg) {
  // q: [B,Hq,Sq,D]; k,v: [B,Hkv,Sk,D] -> {o [B,Hq,Sq,D], lse [B,Hq,Sq] f32}
  // q_seg [B,Sq], kv_seg [B,Sk] int32 (both or neither): the segment mask
  Binding b("fa_gen_fwd", "q", q);
  FaGenShape s = fa_gen_check(b, q, k, v, causal, shift, q_seg, kv_seg);
  auto out = at::empty_like(q);
  auto lse = at::empty({s.B, s.Hq, s.Sq}, q.options().dtype(F32));
  FaGenSeg g = fa_gen_seg(b, s, q, q_seg, kv_seg);
  b.launch(FA_GEN_KERNEL_SEG(fa_gen_fwd_kernel, s),
           dim3((s.Sq + FG_BLK - 1) / FG_BLK, s.Hq, s.B), FG_THREADS, bf16(q), bf16(k),
           bf16(v), bf16_mut(out), lse.data_ptr<float>(), s.Hq, s.Hkv, s.Sq, s.Sk,
           (float)(scale * 1.4426950408889634), causal ? 1 : 0, s.shift, g.q, g.kv,
           g.tiles);
  return {out, lse};
}

std::vector<at::Tensor> fa_gen_bwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                   at::Tensor o, at::Tensor dout, at::Tensor lse,
                                   OptTensor dlse, double scale, bool causal,
                                   int64_t shift, OptTensor q_seg, OptTensor kv_seg) {
  Binding b("fa_gen_bwd", "q", q);
  FaGenShape s = fa_gen_check(b, q, k, v, causal, shift, q_seg, kv_seg);
  b.arg("o", o, BF16, q.sizes());
  b.arg("dout", dout, BF16, q.sizes());
  b.arg("lse", lse, F32, {s.B, s.Hq, s.Sq});
  b.arg("dlse", dlse, F32, {s.B, s.Hq, s.Sq});
  auto delta = at::empty({s.B, s.Hq, s.Sq}, q.options().dtype(F32));
  auto dq = at::empty_like(q);
  auto dk = at::empty_like(k);
  auto dv = at::empty_like(v);
  int64_t rows = (int64_t)s.B * s.Hq * s.Sq;
  FaGenSeg g = fa_gen_seg(b, s, q, q_seg, kv_seg);
  b.launch(FA_GEN_KERNEL(fa_gen_preprocess_kernel, s.D),
           grid_for(rows, 256 / (s.D / 8), 4096), 256, bf16(dout), bf16(o),
           lse.data_ptr<float>(), f32(dlse), delta.data_ptr<float>(), rows);
  b.launch(FA_GEN_KERNEL_SEG(fa_gen_dkdv_kernel, s),
           dim3((s.Sk + FG_BLK - 1) / FG_BLK, s.Hkv, s.B), FG_THREADS, bf16(q), bf16(k),
           bf16(v), bf16(dout), lse.data_ptr<float>(), delta.data_ptr<float>(),
           bf16_mut(dk), bf16_mut(dv), s.Hq, s.Hkv, s.Sq, s.Sk, (float)scale,
           causal ? 1 : 0, s.shift, g.q, g.kv, g.tiles);
  b.launch(FA_GEN_KERNEL_SEG(fa_gen_dq_kernel, s),
           dim3((s.Sq + FG_BLK - 1) / FG_BLK, s.Hq, s.B), FG_THREADS, bf16(q), bf16(k),
           bf16(v), bf16(dout), lse.data_ptr<float>(), delta.data_ptr<float>(),
           bf16_mut(dq), s.Hq, s.Hkv, s.Sq, s.Sk, (float)scale, causal ? 1 : 0,
           s.shift, g.q, g.kv, g.tiles);
  return {dq, dk, dv};
}

// fa_gen_bwd behind the tuned kernels' argument checks (causal, D = 128,
// S % 64 == 0, no dlse)
std::vector<at::Tensor> fa_bwd(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                               at::Tensor dout, at::Tensor lse, double scale) {
  fa_check(Binding("fa_bwd", "q", q), FG_BLK, q, k, v, o, dout, lse);
  TORCH_CHECK(q.is_cuda(), "fa_bwd: argument 'q' expected device=a GPU; got device=", q.device());
  return fa_gen_bwd(q, k, v, o, dout, lse, {}, scale, true, 0, {}, {});
}

// ------------------------------ philox random ------------------------------
using Dims = std::vector<int64_t>;

// Shard descriptor for a local tensor of `numel` elements.
ShardDesc make_desc(const char* fn, const Dims& gshape, const Dims& lshape,
                    const Dims& offset, int64_t flat_offset, bool is_flat,
                    int64_t numel) {
  TORCH_CHECK(gshape.size() <= MAXD && lshape.size() == gshape.size() &&
                  offset.size() == gshape.size(),
              fn, ": gshape, lshape, offset must have one length <= ", MAXD,
              ", got ", gshape.size(), ", ", lshape.size(), ", ", offset.size());
  ShardDesc d{};
  d.ndim = (int)gshape.size();
  int64_t prod = 1;
  for (int i = 0; i < d.ndim; ++i) {
    d.gshape[i] = gshape[i];
    d.lshape[i] = lshape[i];
    d.offset[i] = offset[i];
    prod *= lshape[i];
  }
  TORCH_CHECK(prod == numel, fn, ": prod(lshape) = ", prod,
              " must equal the tensor's numel = ", numel);
  d.flat_offset = flat_offset;
  d.is_flat = is_flat ? 1 : 0;
  return d;
}

// philox_uniform_(.., lo, hi) and philox_normal_(.., mean, std): one dtype dispatch.
template <bool NORMAL>
void philox_fill(at::Tensor out, Dims gshape, Dims lshape, Dims offset,
                 int64_t flat_offset, bool is_flat, int64_t seed, int64_t philox_offset,
                 double p0, double p1) {
  Binding b(NORMAL ? "philox_normal_" : "philox_uniform_", "out", out);
  int64_t n = out.numel();
  auto d = make_desc(b.fn, gshape, lshape, offset, flat_offset, is_flat, n);
  b.arg("out", out, {BF16, F32});
  if (out.scalar_type() == BF16)
    b.launch(NORMAL ? philox_normal_bf16 : philox_uniform_bf16, grid_for(n, 256), 256,
             bf16_mut(out), d, n, (uint64_t)seed, (uint64_t)philox_offset, (float)p0,
             (float)p1);
  else
    b.launch(NORMAL ? philox_normal_f32 : philox_uniform_f32, grid_for(n, 256), 256,
             out.data_ptr<float>(), d, n, (uint64_t)seed, (uint64_t)philox_offset,
             (float)p0, (float)p1);
}

std::vector<at::Tensor> philox_dropout(at::Tensor x, Dims gshape, Dims lshape,
                                       Dims offset, int64_t flat_offset, bool is_flat,
                                       int64_t seed, int64_t philox_offset, double p,
                                       bool need_mask) {
  Binding b("philox_dropout", "x", x);
  TORCH_CHECK(p >= 0.0 && p < 1.0, "philox_dropout: p = ", p, " must be in [0, 1)");
  int64_t n = x.numel();
  auto d = make_desc(b.fn, gshape, lshape, offset, flat_offset, is_flat, n);
  b.arg("x", x, BF16);
  auto out = at::empty_like(x);
  at::Tensor mask;
  if (need_mask) mask = at::empty(x.sizes(), x.options().dtype(at::kByte));
  b.launch(philox_dropout_bf16, grid_for(n, 256), 256, bf16(x), bf16_mut(out),
           need_mask ? mask.data_ptr<unsigned char>() : nullptr, d, n, (uint64_t)seed,
           (uint64_t)philox_offset, (float)p);
  if (need_mask) return {out, mask};
  return {out};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("rmsnorm_bwd", &rmsnorm_bwd, pybind11::arg("dy"), pybind11::arg("x"),
        pybind11::arg("w"), pybind11::arg("rrms"),
        pybind11::arg("dres") = pybind11::none());
  m.def("rmsnorm_res_fwd", &rmsnorm_res_fwd);
  m.def("rope", &rope);
  m.def("rope_qkv_fwd", &rope_qkv_fwd);
  m.def("rope_qkv_bwd", &rope_qkv_bwd);
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("swiglu_packed_fwd", &swiglu_packed_fwd);
  m.def("swiglu_packed_bwd", &swiglu_packed_bwd);
  m.def("ce_fwd", &ce_fwd, pybind11::arg("logits"), pybind11::arg("target"),
        pybind11::arg("ignore_index"), pybind11::arg("vocab_start") = 0,
        pybind11::arg("vocab_total") = -1);
  m.def("ce_bwd", &ce_bwd, pybind11::arg("logits"), pybind11::arg("target"),
        pybind11::arg("lse"), pybind11::arg("dloss"), pybind11::arg("ignore_index"),
        pybind11::arg("inplace"), pybind11::arg("vocab_start") = 0,
        pybind11::arg("vocab_total") = -1);
  m.def("adamw_step", &adamw_step);
  m.def("l2norm_sq", &l2norm_sq);
  m.def("scale_", &scale_);
  m.def("gemm_tn", &gemm_tn, pybind11::arg("a"), pybind11::arg("b"), pybind11::arg("variant") = 0);
  m.def("gemm_tn8", &gemm_tn8, pybind11::arg("a"), pybind11::arg("b"), pybind11::arg("mode") = 0);
  m.def("fa_bwd", &fa_bwd);
  m.def("fa_bwd2", &fa_bwd2, pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("v"),
        pybind11::arg("o"), pybind11::arg("dout"), pybind11::arg("lse"),
        pybind11::arg("scale"), pybind11::arg("fused_dvdk"), pybind11::arg("bshd") = false);
  m.def("fa_fwd", &fa_fwd, pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("v"),
        pybind11::arg("scale"), pybind11::arg("out_bshd") = false);
  m.def("fa_fwd_ablate", &fa_fwd_ablate);
  m.def("fa_gen_fwd", &fa_gen_fwd, pybind11::arg("q"), pybind11::arg("k"),
        pybind11::arg("v"), pybind11::arg("scale"), pybind11::arg("causal"),
        pybind11::arg("shift"), pybind11::arg("q_seg") = pybind11::none(),
        pybind11::arg("kv_seg") = pybind11::none());
  m.def("fa_gen_bwd", &fa_gen_bwd, pybind11::arg("q"), pybind11::arg("k"),
        pybind11::arg("v"), pybind11::arg("o"), pybind11::arg("dout"),
        pybind11::arg("lse"), pybind11::arg("dlse"), pybind11::arg("scale"),
        pybind11::arg("causal"), pybind11::arg("shift"),
        pybind11::arg("q_seg") = pybind11::none(),
        pybind11::arg("kv_seg") = pybind11::none());
  m.def("permlane_probe", &permlane_probe);
  m.def("mfma32_probe", &mfma32_probe);
  m.def("tr_probe", &tr_probe);
  m.def("_relayout_probe", &relayout_probe, pybind11::arg("x"));
  m.def("philox_uniform_", &philox_fill<false>);
  m.def("philox_normal_", &philox_fill<true>);
  m.def("philox_dropout", &philox_dropout);
}
