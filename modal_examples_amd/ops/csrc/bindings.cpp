// Torch extension bindings for the gfx950 kernel suite + the pinned-host
// snapshot engine (K13, SURVEY.md §2.4: the GPU memory-snapshot engine behind
// the reference's cold-start lifecycle, gpu_snapshot.py:41-53 /
// sglang_snapshot.py:303-312).
//
// The kernels themselves live in the sibling .hip files (plain HIP, no torch
// dependency); this is the only file that includes <torch/extension.h>.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <unordered_map>
#include <vector>

// ---- extern "C" launchers from the .hip translation units ----
extern "C" {
// the attention launchers return 0 once launched, non-zero (nothing
// launched) for a configuration they do not support
int fa32_fwd_strided_bf16(const void*, const void*, const void*, void*, float*,
                          int, int, int, int, int, int, float, int,
                          const long long*, hipStream_t);
int fa_bwd_strided_bf16(const void*, const void*, const void*, const void*,
                        const void*, const float*, float*, void*, void*, void*,
                        int, int, int, int, int, int, float, int,
                        const long long*, hipStream_t);
int paged_decode_bf16(const void*, const void*, const void*, const int*,
                      const int*, void*, float*, int, int, int, int, int,
                      int, int, float, int, hipStream_t);
int paged_prefill_bf16(const void*, const void*, const void*, const int*,
                       const int*, const int*, void*, int, int, int, int, int,
                       int, int, float, int, hipStream_t);
void groupnorm_silu_bf16(const void*, void*, float*, const float*,
                         const float*, int, int, long long, int, float, int,
                         hipStream_t);
void groupnorm_silu_nhwc_bf16(const void*, void*, float*, const float*,
                              const float*, int, int, long long, int, float,
                              int, hipStream_t);
void layernorm_bf16(const void*, void*, const float*, const float*, long long,
                    int, float, hipStream_t);
void add_layernorm_bf16(const void*, const void*, void*, void*, const float*,
                        const float*, long long, int, float, hipStream_t);
void add_nhwc_to_nchw_bf16(const void*, const void*, void*, int, int,
                           long long, hipStream_t);
void scaled_softmax_bf16(const void*, void*, long long, int, float,
                         hipStream_t);
void rmsnorm_bf16(const void*, void*, const float*, long long, int, float,
                  hipStream_t);
void cfg_euler_bf16(const void*, const void*, const void*, void*, float, float,
                    long long, hipStream_t);
void silu_mul_bf16(const void*, const void*, void*, long long, hipStream_t);
void geglu_bf16(const void*, const void*, void*, long long, hipStream_t);
void glu_fused_bf16(const void*, void*, long long, long long, int,
                    hipStream_t);
void add_bf16(const void*, const void*, void*, long long, hipStream_t);
void rope_bf16(void*, const float*, const float*, long long, int, int, int,
               long long, long long, long long, const int*, hipStream_t);
void adamw_step(void*, const void*, float*, float*, long long, float, float,
                float, float, float, int, int, hipStream_t);
void gumbel_sample(const float*, unsigned long long*, int*, int, int,
                   float, unsigned long long, hipStream_t);
void sampling_cutoff(const float*, const float*, const int*, const float*,
                     const float*, float*, int, int, hipStream_t);
void gumbel_sample_batch(const float*, const float*, const long long*,
                         const long long*, const float*, unsigned long long*,
                         int*, int, int, hipStream_t);
void softmax_rows(const float*, float*, int, int, hipStream_t);
void scale_in_dev_bf16(const void*, void*, const float*, const long long*,
                       long long, hipStream_t);
void cfg_euler_dev_bf16(const void*, const void*, const void*, void*,
                        const float*, const long long*, float, long long,
                        hipStream_t);
void advance_step(long long*, hipStream_t);
void conv3x3_bf16(const void*, const void*, const void*, const void*,
                  const void*, void*, const float*, const float*, int, int,
                  int, int, int, int, int, int, hipStream_t);
void gn_conv_coeffs_bf16(const void*, float*, const float*, const float*,
                         float*, float*, int, int, int, long long, int, float,
                         hipStream_t);
// the MoE launchers return 0 once launched, non-zero (nothing launched)
// for a shape they do not support
int moe_max_tiles(long long, int, int);
int moe_route_f32(const float*, float*, int*, long long, int, int,
                  hipStream_t);
int moe_ffn_bf16(const void*, const void*, const void*, const float*,
                 const int*, int*, void*, float*, void*, long long, int, int,
                 int, int, hipStream_t);
// linear_w4_plan: the K-slice count of a call, 0 for an unsupported shape;
// linear_w4_bf16 returns 0 once launched, non-zero (nothing launched) else
int linear_w4_plan(long long, int, int, int);
int linear_w4_bf16(const void*, const void*, const void*, float*, void*,
                   long long, int, int, int, hipStream_t);
}

namespace {

hipStream_t cur_stream() {
  return (hipStream_t)c10::hip::getCurrentHIPStream().stream();
}

void check_bf16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// ---------------------------------------------------------------- attention

void check_bhsd(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.dim() == 4, name, " must be [B,H,S,D]");
  TORCH_CHECK(t.stride(3) == 1, name, ": head_dim must be contiguous");
}

struct AttnDims {
  int B, Hq, Hkv, Sq, Sk, D;
};

// The q/k/v checks of both directions; `op` names the entry in the messages.
AttnDims check_qkv(const char* op, const torch::Tensor& q,
                   const torch::Tensor& k, const torch::Tensor& v) {
  check_bhsd(q, "q");
  check_bhsd(k, "k");
  check_bhsd(v, "v");
  AttnDims d{(int)q.size(0), (int)q.size(1), (int)k.size(1), (int)q.size(2),
             (int)k.size(2), (int)q.size(3)};
  TORCH_CHECK(d.D == 64 || d.D == 128, op, ": unsupported head_dim ", d.D,
              " (supported: 64, 128)");
  TORCH_CHECK(k.size(0) == d.B && k.size(3) == d.D && v.sizes() == k.sizes(),
              op, ": k/v must be [B,Hkv,Sk,D] matching q's B and D");
  TORCH_CHECK(d.Hkv > 0 && d.Hq % d.Hkv == 0,
              "GQA requires Hq % Hkv == 0, got Hq=", d.Hq, " Hkv=", d.Hkv);
  return d;
}

// appends the (batch, head, sequence) element strides of t: one AttnStride
// of the launchers' flat stride image (csrc/attention_mfma32.h)
void push_strides(std::vector<long long>& st, const torch::Tensor& t) {
  st.insert(st.end(), {t.stride(0), t.stride(1), t.stride(2)});
}

// The one forward-attention launch: q/k/v are logically [B,H,S,D] with ANY
// batch/head/sequence strides (d contiguous), read straight off the tensors.
// The output is allocated here, [B,H,S,D] contiguous or, for bshd,
// [B,S,H,D] contiguous so callers in sequence-major models (UNet/Llama/
// Whisper blocks) skip every transpose copy around the kernel.  with_lse
// (training) also returns the fp32 log-sum-exp per query row [B,Hq,Sq] that
// the backward recomputes P from.  Unsupported configurations raise here,
// before anything is launched: no key at all (Sk == 0) is an error, no
// query at all (B, Hq or Sq zero) returns the empty tensors without a launch.
// out / lse_out, when given, are written instead of fresh tensors and
// returned: out bf16 of the output's shape with any strides (d contiguous),
// lse_out fp32 [B,Hq,Sq] contiguous.
std::tuple<torch::Tensor, torch::Tensor> attention_fwd(
    const torch::Tensor& q, const torch::Tensor& k, const torch::Tensor& v,
    bool causal, double scale, bool bshd, bool with_lse,
    const c10::optional<torch::Tensor>& out = c10::nullopt,
    const c10::optional<torch::Tensor>& lse_out = c10::nullopt) {
  const AttnDims d = check_qkv("attention", q, k, v);
  TORCH_CHECK(d.Sk >= 1, "attention: Sk must be at least 1, got Sk=", d.Sk,
              " (a query with no key has no softmax)");
  const std::vector<int64_t> o_shape =
      bshd ? std::vector<int64_t>{d.B, d.Sq, d.Hq, d.D}
           : std::vector<int64_t>{d.B, d.Hq, d.Sq, d.D};
  torch::Tensor o;
  if (out.has_value()) {
    o = *out;
    TORCH_CHECK(o.device() == q.device() && o.scalar_type() == torch::kBFloat16 &&
                o.sizes() == torch::IntArrayRef(o_shape) &&
                (o.numel() == 0 || o.stride(3) == 1),
                "attention: out must be bf16 on the GPU with the output's "
                "shape ", torch::IntArrayRef(o_shape), " and head_dim "
                "contiguous");
  } else {
    o = torch::empty(o_shape, q.options());
  }
  torch::Tensor lse;
  if (with_lse) {
    if (lse_out.has_value()) {
      lse = *lse_out;
      TORCH_CHECK(lse.device() == q.device() && lse.scalar_type() == torch::kFloat32 &&
                  lse.dim() == 3 && lse.size(0) == d.B &&
                  lse.size(1) == d.Hq && lse.size(2) == d.Sq &&
                  lse.is_contiguous(),
                  "attention: lse must be fp32 [B,Hq,Sq] contiguous");
    } else {
      lse = torch::empty({d.B, d.Hq, d.Sq},
                         q.options().dtype(torch::kFloat32));
    }
  }
  if (o.numel() == 0) return {o, lse};  // a zero grid dimension is no launch
  std::vector<long long> st;
  for (const auto& t : {q, k, v, bshd ? o.transpose(1, 2) : o})
    push_strides(st, t);
  int rc = fa32_fwd_strided_bf16(
      q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
      with_lse ? lse.data_ptr<float>() : nullptr, d.B, d.Hq, d.Hkv, d.Sq,
      d.Sk, d.D, (float)scale, causal ? 1 : 0, st.data(), cur_stream());
  TORCH_CHECK(rc == 0, "attention: configuration not supported by the kernel "
              "(head_dim must be 64 or 128 and Hq a multiple of Hkv; got D=",
              d.D, " Hq=", d.Hq, " Hkv=", d.Hkv, ")");
  return {o, lse};
}

torch::Tensor attention(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                        bool causal, double scale) {
  check_bf16(q, "q");
  check_bf16(k, "k");
  check_bf16(v, "v");
  return std::get<0>(attention_fwd(q, k, v, causal, scale, false, false));
}

torch::Tensor attention_bshd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                             bool causal, double scale) {
  return std::get<0>(attention_fwd(q, k, v, causal, scale, true, false));
}

std::tuple<torch::Tensor, torch::Tensor> attention_fwd_lse(
    torch::Tensor q, torch::Tensor k, torch::Tensor v, bool causal,
    double scale, c10::optional<torch::Tensor> out,
    c10::optional<torch::Tensor> lse) {
  return attention_fwd(q, k, v, causal, scale, false, true, out, lse);
}

std::tuple<torch::Tensor, torch::Tensor> attention_fwd_lse_bshd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v, bool causal,
    double scale, c10::optional<torch::Tensor> out,
    c10::optional<torch::Tensor> lse) {
  return attention_fwd(q, k, v, causal, scale, true, true, out, lse);
}

torch::Tensor paged_decode(torch::Tensor q, torch::Tensor kc, torch::Tensor vc,
                           c10::optional<torch::Tensor> block_table,
                           torch::Tensor seq_lens, int64_t block_size,
                           double scale) {
  check_bf16(q, "q");
  // KV cache: bf16, or OCP e4m3 fp8 (the vllm_low_latency FP8-serving role
  // — halves KV bytes per decoded token)
  const bool kv_fp8 = kc.scalar_type() == torch::kFloat8_e4m3fn;
  TORCH_CHECK(kv_fp8 || kc.scalar_type() == torch::kBFloat16,
              "k_cache must be bf16 or float8_e4m3fn");
  TORCH_CHECK(vc.scalar_type() == kc.scalar_type(), "kv cache dtype mismatch");
  TORCH_CHECK(kc.is_contiguous() && vc.is_contiguous());
  TORCH_CHECK(q.dim() == 3 && kc.dim() == 4, "q must be [B,Hq,D], k_cache "
              "[blocks,Hkv,block_size,D] or [B,Hkv,S,D]");
  int B = q.size(0), Hq = q.size(1), D = q.size(2);
  // cache is [blocks, Hkv, block_size, D], or [B, Hkv, S, D] without a table
  int Hkv = kc.size(1), max_blocks = 0;
  TORCH_CHECK(D == 64 || D == 128, "paged_decode: unsupported head_dim ", D,
              " (supported: 64, 128)");
  TORCH_CHECK(kc.size(3) == D, "paged_decode: k_cache head_dim ", kc.size(3),
              " != q head_dim ", D);
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, "GQA requires Hq % Hkv == 0, got Hq=",
              Hq, " Hkv=", Hkv);
  TORCH_CHECK(Hq / Hkv <= 8, "paged_decode: unsupported GQA group Hq/Hkv = ",
              Hq / Hkv, " (supported: 1..8)");
  const int* bt_ptr = nullptr;
  if (block_table.has_value()) {
    max_blocks = block_table->size(1);
    bt_ptr = block_table->data_ptr<int>();
  } else {
    block_size = kc.size(2);
  }
  auto o = torch::empty_like(q);
  // flash-decoding split: fill the chip when B*Hkv is small; cap splits by
  // the longest representable sequence so chunks stay >=256 kv rows
  long long s_bound = block_table.has_value()
      ? (long long)max_blocks * block_size : (long long)kc.size(2);
  int splits = 1;
  // fill the chip for latency-path decodes: allow chunks down to 128 kv
  // rows (B1/Hkv8/S4096 was 128 workgroups = half the CUs idle)
  while (B * Hkv * splits < 512 && (long long)splits * 128 < s_bound &&
         splits < 64)
    splits *= 2;
  torch::Tensor ws;
  float* ws_ptr = nullptr;
  if (splits > 1) {
    ws = torch::empty({(long long)B * Hq * splits * (D + 2)},
                      q.options().dtype(torch::kFloat32));
    ws_ptr = ws.data_ptr<float>();
  }
  int rc = paged_decode_bf16(q.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                             bt_ptr, seq_lens.data_ptr<int>(), o.data_ptr(),
                             ws_ptr, B, Hq, Hkv, D, (int)block_size,
                             max_blocks, splits, (float)scale, kv_fp8 ? 1 : 0,
                             cur_stream());
  TORCH_CHECK(rc == 0, "paged_decode: configuration not supported by the "
              "kernel (head_dim must be 64 or 128, Hq a multiple of Hkv and "
              "Hq/Hkv in 1..8; got D=", D, " Hq=", Hq, " Hkv=", Hkv, ")");
  return o;
}

// Causal attention of a ragged batch of new query tokens q [T,Hq,D] (rows
// cu_q[b]..cu_q[b+1] belong to sequence b) against a paged cache that already
// holds their K/V; seq_lens[b] counts the new tokens too.  Every check raises
// before anything is launched.  What only the device knows stays a
// precondition (csrc/attention_prefill_paged.hip): seq_lens[b] >= the
// sequence's query count, valid table entries below seq_lens[b], and
// max_q_len >= the longest query run.
torch::Tensor paged_prefill(torch::Tensor q, torch::Tensor kc, torch::Tensor vc,
                            torch::Tensor block_table, torch::Tensor cu_q,
                            torch::Tensor seq_lens, int64_t block_size,
                            double scale, int64_t max_q_len) {
  check_bf16(q, "q");
  TORCH_CHECK(q.dim() == 3, "paged_prefill: q must be [T,Hq,D]");
  const bool kv_fp8 = kc.scalar_type() == torch::kFloat8_e4m3fn;
  TORCH_CHECK(kv_fp8 || kc.scalar_type() == torch::kBFloat16,
              "k_cache must be bf16 or float8_e4m3fn");
  TORCH_CHECK(vc.scalar_type() == kc.scalar_type(), "kv cache dtype mismatch");
  TORCH_CHECK(kc.dim() == 4 && vc.sizes() == kc.sizes() &&
                  kc.is_contiguous() && vc.is_contiguous(),
              "paged_prefill: k_cache/v_cache must be contiguous "
              "[blocks,Hkv,block_size,D] of one shape");
  const int64_t T = q.size(0);
  const int Hq = q.size(1), D = q.size(2), Hkv = kc.size(1);
  TORCH_CHECK(D == 64 || D == 128, "paged_prefill: unsupported head_dim ", D,
              " (supported: 64, 128)");
  TORCH_CHECK(kc.size(3) == D, "paged_prefill: k_cache head_dim ", kc.size(3),
              " != q head_dim ", D);
  TORCH_CHECK(Hkv > 0 && Hq % Hkv == 0, "GQA requires Hq % Hkv == 0, got Hq=",
              Hq, " Hkv=", Hkv);
  TORCH_CHECK(block_size > 0 && kc.size(2) == block_size,
              "paged_prefill: block_size must be positive and the cache's "
              "third dim, got block_size=", block_size, " cache ", kc.sizes());
  TORCH_CHECK(seq_lens.scalar_type() == torch::kInt32 && seq_lens.dim() == 1 &&
                  seq_lens.is_contiguous(),
              "paged_prefill: seq_lens must be int32 [B] contiguous");
  const int64_t B = seq_lens.size(0);
  TORCH_CHECK(block_table.scalar_type() == torch::kInt32 &&
                  block_table.dim() == 2 && block_table.size(0) == B &&
                  block_table.is_contiguous(),
              "paged_prefill: block_table must be int32 [B=", B,
              ", max_blocks] contiguous, got ", block_table.sizes());
  TORCH_CHECK(cu_q.scalar_type() == torch::kInt32 && cu_q.dim() == 1 &&
                  cu_q.size(0) == B + 1 && cu_q.is_contiguous(),
              "paged_prefill: cu_q must be int32 [B+1=", B + 1, "], got ",
              cu_q.sizes());
  for (const torch::Tensor* t : {&kc, &vc, &block_table, &cu_q, &seq_lens})
    TORCH_CHECK(t->device() == q.device(),
                "paged_prefill: all tensors must be on q's device");
  auto o = torch::empty_like(q);
  if (T == 0) return o;  // nothing to attend: max_q_len=None arrives as T = 0
  TORCH_CHECK(max_q_len >= 1, "paged_prefill: max_q_len must be at least 1, "
              "got ", max_q_len);
  TORCH_CHECK(B >= 1, "paged_prefill: ", T, " query rows but no sequence");
  max_q_len = std::min<int64_t>(max_q_len, T);  // no run is longer than T
  int rc = paged_prefill_bf16(
      q.data_ptr(), kc.data_ptr(), vc.data_ptr(), block_table.data_ptr<int>(),
      cu_q.data_ptr<int>(), seq_lens.data_ptr<int>(), o.data_ptr(), (int)B, Hq,
      Hkv, D, (int)block_size, (int)block_table.size(1), (int)max_q_len,
      (float)scale, kv_fp8 ? 1 : 0, cur_stream());
  TORCH_CHECK(rc == 0, "paged_prefill: configuration not supported by the "
              "kernel (head_dim must be 64 or 128, Hq a multiple of Hkv, B "
              "and Hq at most 65535; got D=", D, " Hq=", Hq, " Hkv=", Hkv,
              " B=", B, ")");
  return o;
}

// Attention backward into caller-provided dq/dk/dv.  Everything is logically
// [B,H,S,D] with any batch/head/sequence strides (d contiguous); every check
// raises before anything is launched.
void attention_bwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                   torch::Tensor o, torch::Tensor lse, torch::Tensor dout,
                   torch::Tensor dq, torch::Tensor dk, torch::Tensor dv,
                   bool causal, double scale) {
  const AttnDims d = check_qkv("attention_bwd", q, k, v);
  const int B = d.B, Hq = d.Hq, Hkv = d.Hkv, Sq = d.Sq, Sk = d.Sk, D = d.D;
  check_bhsd(o, "o");
  check_bhsd(dout, "dout");
  check_bhsd(dq, "dq");
  check_bhsd(dk, "dk");
  check_bhsd(dv, "dv");
  TORCH_CHECK(B >= 1 && Sq >= 1 && Sk >= 1, "attention_bwd: empty input");
  TORCH_CHECK(o.sizes() == q.sizes() && dout.sizes() == q.sizes(),
              "attention_bwd: o and dout must have q's shape");
  TORCH_CHECK(dq.sizes() == q.sizes() && dk.sizes() == k.sizes() &&
              dv.sizes() == v.sizes(),
              "attention_bwd: dq/dk/dv must have the shapes of q/k/v");
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == torch::kFloat32 &&
              lse.dim() == 3 && lse.size(0) == B && lse.size(1) == Hq &&
              lse.size(2) == Sq && lse.is_contiguous(),
              "attention_bwd: lse must be fp32 [B,Hq,Sq] contiguous");
  TORCH_CHECK(!causal || Sk >= Sq, "attention_bwd: causal requires Sk >= Sq, "
              "got Sq=", Sq, " Sk=", Sk);
  auto delta = torch::empty_like(lse);
  std::vector<long long> st;
  for (const auto& t : {q, k, v, o, dout, dq, dk, dv}) push_strides(st, t);
  int rc = fa_bwd_strided_bf16(
      q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), dout.data_ptr(),
      lse.data_ptr<float>(), delta.data_ptr<float>(), dq.data_ptr(),
      dk.data_ptr(), dv.data_ptr(), B, Hq, Hkv, Sq, Sk, D, (float)scale,
      causal ? 1 : 0, st.data(), cur_stream());
  TORCH_CHECK(rc == 0, "attention_bwd: configuration not supported by the "
              "kernel (got D=", D, " Hq=", Hq, " Hkv=", Hkv, " Sq=", Sq,
              " Sk=", Sk, " causal=", causal, ")");
}

// ---------------------------------------------------------------- norms

torch::Tensor groupnorm_silu(torch::Tensor x, torch::Tensor gamma,
                             torch::Tensor beta, int64_t groups, double eps,
                             bool do_silu) {
  check_bf16(x, "x");
  TORCH_CHECK(x.dim() == 4, "x must be NCHW");
  int N = x.size(0), C = x.size(1);
  long long HW = (long long)x.size(2) * x.size(3);
  auto y = torch::empty_like(x);
  auto ws = torch::zeros({N * groups * 2},
                         x.options().dtype(torch::kFloat32));
  groupnorm_silu_bf16(x.data_ptr(), y.data_ptr(), ws.data_ptr<float>(),
                      gamma.data_ptr<float>(), beta.data_ptr<float>(), N, C,
                      HW, (int)groups, (float)eps, do_silu ? 1 : 0,
                      cur_stream());
  return y;
}

torch::Tensor layernorm(torch::Tensor x, torch::Tensor gamma,
                        torch::Tensor beta, double eps) {
  check_bf16(x, "x");
  int D = x.size(-1);
  long long rows = x.numel() / D;
  auto y = torch::empty_like(x);
  layernorm_bf16(x.data_ptr(), y.data_ptr(), gamma.data_ptr<float>(),
                 beta.data_ptr<float>(), rows, D, (float)eps, cur_stream());
  return y;
}

// a per-channel fp32 parameter vector of the fused glue ops below
void check_f32_param(const char* op, const torch::Tensor& t, const char* name,
                     int64_t n) {
  TORCH_CHECK(t.is_cuda(), op, ": ", name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kFloat, op, ": ", name,
              " must be fp32");
  TORCH_CHECK(t.is_contiguous() && t.dim() == 1 && t.numel() == n, op, ": ",
              name, " must be a contiguous vector of ", n, " elements, got ",
              t.sizes());
}

void check_same_device(const char* op, const torch::Tensor& a,
                       const torch::Tensor& b, const char* name) {
  TORCH_CHECK(a.device() == b.device(), op, ": ", name, " is on ", b.device(),
              ", expected ", a.device());
}

// GroupNorm(+SiLU) of an NCHW tensor, written as [N, H*W, C] (NHWC flattened
// over the pixels): groupnorm_silu(x).permute(0,2,3,1).reshape(N, HW, C)
// without the transposing copy.  Everything is checked before the launch.
torch::Tensor groupnorm_silu_nhwc(torch::Tensor x, torch::Tensor gamma,
                                  torch::Tensor beta, int64_t groups,
                                  double eps, bool do_silu) {
  const char* op = "groupnorm_silu_nhwc";
  check_bf16(x, "x");
  TORCH_CHECK(x.dim() == 4, op, ": x must be NCHW, got ", x.dim(), " dims");
  const int64_t N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  TORCH_CHECK(groups >= 1 && C >= 1 && C % groups == 0, op,
              ": groups must be at least 1 and divide C, got groups=", groups,
              " C=", C);
  check_f32_param(op, gamma, "gamma", C);
  check_f32_param(op, beta, "beta", C);
  check_same_device(op, x, gamma, "gamma");
  check_same_device(op, x, beta, "beta");
  // grid z is the image, grid x the pixel tile; N*groups indexes the sums
  TORCH_CHECK(N <= 65535 && HW < (1ll << 31) && C < (1ll << 22) &&
                  N * groups < (1ll << 20),
              op, ": too large for the kernel (N <= 65535, H*W < 2^31, "
              "C < 2^22, N*groups < 2^20), got x ", x.sizes());
  auto y = torch::empty({N, HW, C}, x.options());
  auto ws = torch::zeros({N * groups * 2}, x.options().dtype(torch::kFloat32));
  groupnorm_silu_nhwc_bf16(x.data_ptr(), y.data_ptr(), ws.data_ptr<float>(),
                           gamma.data_ptr<float>(), beta.data_ptr<float>(),
                           (int)N, (int)C, HW, (int)groups, (float)eps,
                           do_silu ? 1 : 0, cur_stream());
  return y;
}

// (x + y, LayerNorm(x + y)) over the last dimension, from one read of x, y.
std::vector<torch::Tensor> add_layernorm(torch::Tensor x, torch::Tensor y,
                                         torch::Tensor gamma,
                                         torch::Tensor beta, double eps) {
  const char* op = "add_layernorm";
  check_bf16(x, "x");
  check_bf16(y, "y");
  check_same_device(op, x, y, "y");
  TORCH_CHECK(x.dim() >= 1 && x.sizes() == y.sizes(), op,
              ": x and y must have one shape, got ", x.sizes(), " and ",
              y.sizes());
  const int64_t D = x.size(-1);
  TORCH_CHECK(D >= 8 && D % 8 == 0 && D < (1ll << 31), op,
              ": the last dimension must be a positive multiple of 8 (rows "
              "start on 16-byte boundaries), got ", D);
  check_f32_param(op, gamma, "gamma", D);
  check_f32_param(op, beta, "beta", D);
  check_same_device(op, x, gamma, "gamma");
  check_same_device(op, x, beta, "beta");
  const int64_t rows = x.numel() / D;
  TORCH_CHECK((rows + 3) / 4 < (1ll << 31), op, ": too many rows: ", rows);
  auto s = torch::empty_like(x);
  auto ln = torch::empty_like(x);
  add_layernorm_bf16(x.data_ptr(), y.data_ptr(), s.data_ptr(), ln.data_ptr(),
                     gamma.data_ptr<float>(), beta.data_ptr<float>(), rows,
                     (int)D, (float)eps, cur_stream());
  return {s, ln};
}

torch::Tensor rmsnorm(torch::Tensor x, torch::Tensor gamma, double eps) {
  check_bf16(x, "x");
  int D = x.size(-1);
  TORCH_CHECK(D % 8 == 0, "rmsnorm needs D % 8 == 0");
  long long rows = x.numel() / D;
  auto y = torch::empty_like(x);
  rmsnorm_bf16(x.data_ptr(), y.data_ptr(), gamma.data_ptr<float>(), rows, D,
               (float)eps, cur_stream());
  return y;
}

// ---------------------------------------------------------------- elementwise

torch::Tensor cfg_euler(torch::Tensor xt, torch::Tensor eps_c,
                        c10::optional<torch::Tensor> eps_u, double guidance,
                        double dsigma) {
  check_bf16(xt, "x_t");
  auto xn = torch::empty_like(xt);
  cfg_euler_bf16(xt.data_ptr(), eps_c.data_ptr(),
                 eps_u.has_value() ? eps_u->data_ptr() : nullptr,
                 xn.data_ptr(), (float)guidance, (float)dsigma, xt.numel(),
                 cur_stream());
  return xn;
}

torch::Tensor silu_mul(torch::Tensor a, torch::Tensor b) {
  check_bf16(a, "a");
  auto y = torch::empty_like(a);
  silu_mul_bf16(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(),
                cur_stream());
  return y;
}

torch::Tensor geglu(torch::Tensor a, torch::Tensor b) {
  check_bf16(a, "a");
  auto y = torch::empty_like(a);
  geglu_bf16(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), cur_stream());
  return y;
}

// act(src[..., :I]) * src[..., I:] without slicing copies — src is the
// fused gate_up / GEGLU projection output [rows, 2I]
torch::Tensor glu_fused(torch::Tensor src, bool gelu) {
  check_bf16(src, "src");
  long long inner = src.size(-1) / 2;
  TORCH_CHECK(src.size(-1) % 2 == 0 && inner % 8 == 0,
              "inner dim must be even and 8-aligned");
  long long rows = src.numel() / (2 * inner);
  auto sizes = src.sizes().vec();
  sizes.back() = inner;
  auto y = torch::empty(sizes, src.options());
  glu_fused_bf16(src.data_ptr(), y.data_ptr(), rows, inner, gelu ? 1 : 0,
                 cur_stream());
  return y;
}

torch::Tensor add_residual(torch::Tensor a, torch::Tensor b) {
  check_bf16(a, "a");
  auto y = torch::empty_like(a);
  add_bf16(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), cur_stream());
  return y;
}

// res [N,C,H,W] + h [N,H*W,C] -> [N,C,H,W]: the NHWC result of a
// sequence-major section joins its NCHW residual in one pass.
torch::Tensor add_nhwc_to_nchw(torch::Tensor res, torch::Tensor h) {
  const char* op = "add_nhwc_to_nchw";
  check_bf16(res, "res");
  check_bf16(h, "h");
  check_same_device(op, res, h, "h");
  TORCH_CHECK(res.dim() == 4, op, ": res must be NCHW, got ", res.dim(),
              " dims");
  const int64_t N = res.size(0), C = res.size(1),
                HW = res.size(2) * res.size(3);
  TORCH_CHECK(h.dim() == 3 && h.size(0) == N && h.size(1) == HW &&
                  h.size(2) == C,
              op, ": h must be [N, H*W, C] = [", N, ", ", HW, ", ", C,
              "], got ", h.sizes());
  TORCH_CHECK(N <= 65535 && HW < (1ll << 31) && C < (1ll << 22), op,
              ": too large for the kernel (N <= 65535, H*W < 2^31, C < 2^22), "
              "got res ", res.sizes());
  auto out = torch::empty_like(res);
  add_nhwc_to_nchw_bf16(res.data_ptr(), h.data_ptr(), out.data_ptr(), (int)N,
                        (int)C, HW, cur_stream());
  return out;
}

// softmax((s * scale).float(), -1).to(bf16) over the last dimension.
torch::Tensor scaled_softmax(torch::Tensor s, double scale) {
  const char* op = "scaled_softmax";
  check_bf16(s, "s");
  TORCH_CHECK(s.dim() >= 1, op, ": s must have at least one dimension");
  const int64_t V = s.size(-1);
  TORCH_CHECK(V >= 8 && V % 8 == 0 && V < (1ll << 31), op,
              ": the last dimension must be a positive multiple of 8, got ",
              V);
  const int64_t rows = s.numel() / V;
  TORCH_CHECK(rows < (1ll << 31), op, ": too many rows: ", rows);
  auto y = torch::empty_like(s);
  scaled_softmax_bf16(s.data_ptr(), y.data_ptr(), rows, (int)V, (float)scale,
                      cur_stream());
  return y;
}

void rope_(torch::Tensor qk, torch::Tensor cosv, torch::Tensor sinv,
           c10::optional<torch::Tensor> positions) {
  TORCH_CHECK(qk.is_cuda() && qk.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(qk.dim() == 4 && qk.stride(3) == 1,
              "qk must be [B,H,S,D] with contiguous head_dim");
  long long B = qk.size(0);
  int H = qk.size(1), S = qk.size(2), D = qk.size(3);
  if (positions.has_value())
    TORCH_CHECK(positions->numel() == B * S || positions->numel() == S,
                "positions must be [B*S] (or [S] with B==1)");
  rope_bf16(qk.data_ptr(), cosv.data_ptr<float>(), sinv.data_ptr<float>(), B,
            H, S, D, qk.stride(0), qk.stride(1), qk.stride(2),
            positions.has_value() ? positions->data_ptr<int>() : nullptr,
            cur_stream());
}

void adamw_(torch::Tensor p, torch::Tensor g, torch::Tensor m, torch::Tensor v,
            double lr, double beta1, double beta2, double eps, double wd,
            int64_t step) {
  TORCH_CHECK(p.is_cuda() && p.is_contiguous(), "p must be contiguous GPU");
  bool bf16 = p.scalar_type() == torch::kBFloat16;
  adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr<float>(),
             v.data_ptr<float>(), p.numel(), (float)lr, (float)beta1,
             (float)beta2, (float)eps, (float)wd, (int)step, bf16 ? 1 : 0,
             cur_stream());
}

// ---------------------------------------------------------------- conv (K3)

void check_f32_vec(const torch::Tensor& t, const char* name, int64_t n,
                   const char* len) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kFloat, name, " must be fp32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.numel() == n, name, " must have ", len, " = ", n,
              " elements, got ", t.numel());
}

struct ConvDims {
  int N, C, H, W, Ho, Wo, Kpad, C16;
};

// The argument checks of both conv entries, all on the host and before any
// launch; `op` names the entry in the messages.  The kernel stages whole
// 64 x 16 weight tiles and reads bias[k] and residual[o] unguarded, so a
// short bias or a mis-packed weight has to stop here.
ConvDims check_conv(const char* op, const torch::Tensor& x,
                    const torch::Tensor& wr, const torch::Tensor& bias,
                    const c10::optional<torch::Tensor>& residual, int64_t K,
                    bool upsample) {
  check_bf16(x, "x");
  check_bf16(wr, "wr");
  TORCH_CHECK(x.dim() == 4, op, ": x must be NCHW, got ", x.dim(), " dims");
  TORCH_CHECK(wr.dim() == 3 && wr.size(0) == 9 && wr.size(1) > 0 &&
                  wr.size(2) > 0 && wr.size(1) % 64 == 0 &&
                  wr.size(2) % 16 == 0,
              op, ": wr must be [9, Kpad, C16] (repacked 3x3 weights) with "
              "Kpad % 64 == 0 and C16 % 16 == 0, got ", wr.sizes());
  ConvDims d{(int)x.size(0), (int)x.size(1), (int)x.size(2), (int)x.size(3),
             0, 0, (int)wr.size(1), (int)wr.size(2)};
  d.Ho = upsample ? d.H * 2 : d.H;
  d.Wo = upsample ? d.W * 2 : d.W;
  TORCH_CHECK(K >= 1, op, ": K must be at least 1, got ", K);
  TORCH_CHECK(K <= d.Kpad && d.C <= d.C16, op,
              ": weight pack smaller than conv (K=", K, " > Kpad=", d.Kpad,
              " or C=", d.C, " > C16=", d.C16, ")");
  // The kernel addresses one input image, one 64-plane output slab and the
  // packed weights with 32-bit byte offsets.
  TORCH_CHECK((int64_t)d.C16 * d.H * d.W < (1ll << 30) &&
                  64ll * d.Ho * d.Wo < (1ll << 31) &&
                  9ll * d.Kpad * d.C16 < (1ll << 31),
              op, ": too large for the kernel's 32-bit offsets (C16*H*W must "
              "stay below 2^30, 64*Ho*Wo and 9*Kpad*C16 below 2^31), got x ",
              x.sizes(), " wr ", wr.sizes());
  check_f32_vec(bias, "bias", K, "K");
  if (residual.has_value()) {
    check_bf16(*residual, "residual");
    TORCH_CHECK(residual->dim() == 4 && residual->size(0) == d.N &&
                    residual->size(1) == K && residual->size(2) == d.Ho &&
                    residual->size(3) == d.Wo,
                op, ": residual shape mismatch: ", residual->sizes(),
                " against output [", d.N, ", ", K, ", ", d.Ho, ", ", d.Wo, "]");
  }
  return d;
}

// addend [N, K] bf16 is added per (image, output channel) after the conv's
// own bf16 rounding; it excludes a residual (no caller needs the pair).
torch::Tensor conv3x3(torch::Tensor x, torch::Tensor wr, torch::Tensor bias,
                      c10::optional<torch::Tensor> residual, int64_t K,
                      bool upsample, c10::optional<torch::Tensor> addend) {
  const ConvDims d = check_conv("conv3x3", x, wr, bias, residual, K, upsample);
  if (addend.has_value()) {
    TORCH_CHECK(!residual.has_value(),
                "conv3x3: addend and residual cannot be combined");
    check_bf16(*addend, "addend");
    TORCH_CHECK(addend->device() == x.device(), "conv3x3: addend is on ",
                addend->device(), ", x on ", x.device());
    TORCH_CHECK(addend->dim() == 2 && addend->size(0) == d.N &&
                    addend->size(1) == K,
                "conv3x3: addend must be [N, K] = [", d.N, ", ", K, "], got ",
                addend->sizes());
  }
  auto out = torch::empty({d.N, K, d.Ho, d.Wo}, x.options());
  conv3x3_bf16(x.data_ptr(), wr.data_ptr(), bias.data_ptr(),
               residual.has_value() ? residual->data_ptr() : nullptr,
               addend.has_value() ? addend->data_ptr() : nullptr,
               out.data_ptr(), nullptr, nullptr, d.N, d.C, d.Ho, d.Wo, (int)K,
               d.C16, d.Kpad, upsample ? 1 : 0, cur_stream());
  return out;
}

// GroupNorm+SiLU fused INTO the conv's staging read: one stats pass over x,
// per-(n,c) coefficients, then the conv applies silu(x*sc+sh) while staging.
torch::Tensor conv3x3_gn(torch::Tensor x, torch::Tensor wr, torch::Tensor bias,
                         c10::optional<torch::Tensor> residual, int64_t K,
                         bool upsample, torch::Tensor gamma,
                         torch::Tensor beta, int64_t groups, double eps) {
  const ConvDims d =
      check_conv("conv3x3_gn", x, wr, bias, residual, K, upsample);
  check_f32_vec(gamma, "gamma", d.C, "C");
  check_f32_vec(beta, "beta", d.C, "C");
  TORCH_CHECK(groups >= 1 && d.C % groups == 0,
              "conv3x3_gn: groups must be at least 1 and divide C, got groups=",
              groups, " C=", d.C);
  const int N = d.N, C16 = d.C16;
  long long HW = (long long)d.H * d.W;
  auto fopt = x.options().dtype(torch::kFloat32);
  auto ws = torch::zeros({(long long)N * groups * 2}, fopt);
  auto scale = torch::empty({(long long)N * C16}, fopt);
  auto shift = torch::empty({(long long)N * C16}, fopt);
  gn_conv_coeffs_bf16(x.data_ptr(), ws.data_ptr<float>(),
                      gamma.data_ptr<float>(), beta.data_ptr<float>(),
                      scale.data_ptr<float>(), shift.data_ptr<float>(), N, d.C,
                      C16, HW, (int)groups, (float)eps, cur_stream());
  auto out = torch::empty({N, K, d.Ho, d.Wo}, x.options());
  conv3x3_bf16(x.data_ptr(), wr.data_ptr(), bias.data_ptr(),
               residual.has_value() ? residual->data_ptr() : nullptr,
               nullptr, out.data_ptr(), scale.data_ptr<float>(),
               shift.data_ptr<float>(), N, d.C, d.Ho, d.Wo, (int)K, C16,
               d.Kpad, upsample ? 1 : 0, cur_stream());
  return out;
}

// ---------------------------------------------------------------- MoE FFN
// Supported: E <= 128, 1 <= top_k <= min(E, 8), dim and ffn_dim multiples of
// 64, any N >= 1.  Every check raises before anything is launched; every
// workspace size depends on shapes only, so both entries capture into a graph.

std::tuple<torch::Tensor, torch::Tensor> moe_route(torch::Tensor logits,
                                                   int64_t top_k) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == torch::kFloat32 &&
                  logits.dim() == 2 && logits.is_contiguous(),
              "moe_route: logits must be fp32 [N,E] contiguous on GPU");
  const int64_t N = logits.size(0), E = logits.size(1);
  TORCH_CHECK(N >= 1, "moe_route: logits has no rows");
  TORCH_CHECK(E >= 1 && E <= 128, "moe_route: logits has E=", E,
              " experts (supported: 1..128)");
  TORCH_CHECK(top_k >= 1 && top_k <= 8 && top_k <= E, "moe_route: top_k=",
              top_k, " (supported: 1..min(E, 8), E=", E, ")");
  auto w = torch::empty({N, top_k}, logits.options());
  auto idx = torch::empty({N, top_k}, logits.options().dtype(torch::kInt32));
  int rc = moe_route_f32(logits.data_ptr<float>(), w.data_ptr<float>(),
                         idx.data_ptr<int>(), N, (int)E, (int)top_k,
                         cur_stream());
  TORCH_CHECK(rc == 0, "moe_route: logits shape ", logits.sizes(),
              " with top_k=", top_k, " not supported by the kernel");
  return {w, idx};
}

// x [N,d], gate_up [E,2F,d], down [E,d,F] bf16; weights fp32 / idx int32
// [N,k], idx in [0,E) and distinct per token (a precondition: only the
// device sees the values).  Returns [N,d] bf16.
torch::Tensor moe_ffn(torch::Tensor x, torch::Tensor gate_up,
                      torch::Tensor down, torch::Tensor weights,
                      torch::Tensor idx) {
  check_bf16(x, "x");
  check_bf16(gate_up, "gate_up");
  check_bf16(down, "down");
  TORCH_CHECK(x.dim() == 2 && gate_up.dim() == 3 && down.dim() == 3,
              "moe_ffn: x must be [N,dim], gate_up [E,2*ffn_dim,dim], down "
              "[E,dim,ffn_dim]");
  const int64_t N = x.size(0), d = x.size(1), E = gate_up.size(0),
                F = down.size(2);
  TORCH_CHECK(N >= 1, "moe_ffn: x has no rows");
  TORCH_CHECK(d >= 64 && d % 64 == 0, "moe_ffn: x has dim=", d,
              " (must be a multiple of 64)");
  TORCH_CHECK(F >= 64 && F % 64 == 0, "moe_ffn: down has ffn_dim=", F,
              " (must be a multiple of 64)");
  TORCH_CHECK(E >= 1 && E <= 128, "moe_ffn: gate_up has E=", E,
              " experts (supported: 1..128)");
  TORCH_CHECK(gate_up.size(1) == 2 * F && gate_up.size(2) == d &&
                  down.size(0) == E && down.size(1) == d,
              "moe_ffn: gate_up ", gate_up.sizes(), " / down ", down.sizes(),
              " do not match [E,2*ffn_dim,dim] / [E,dim,ffn_dim] with dim=",
              d);
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == torch::kInt32 &&
                  idx.dim() == 2 && idx.size(0) == N && idx.is_contiguous(),
              "moe_ffn: idx must be int32 [N,top_k] contiguous on GPU");
  const int64_t k = idx.size(1);
  TORCH_CHECK(k >= 1 && k <= 8 && k <= E, "moe_ffn: idx has top_k=", k,
              " (supported: 1..min(E, 8), E=", E, ")");
  TORCH_CHECK(weights.is_cuda() && weights.scalar_type() == torch::kFloat32 &&
                  weights.sizes() == idx.sizes() && weights.is_contiguous(),
              "moe_ffn: weights must be fp32 [N,top_k] contiguous on GPU");
  for (const torch::Tensor* t : {&gate_up, &down, &weights, &idx})
    TORCH_CHECK(t->device() == x.device(),
                "moe_ffn: all tensors must be on x's device");
  TORCH_CHECK(N * k < (1ll << 30) && N * k * d < (1ll << 40),
              "moe_ffn: x has too many rows (N=", N, ")");
  const int64_t tiles = moe_max_tiles(N, (int)k, (int)E);
  auto iopt = x.options().dtype(torch::kInt32);
  auto sched = torch::empty({tiles * 32 + tiles + 1}, iopt);
  auto h = torch::empty({tiles * 32, F}, x.options());
  auto y = torch::empty({N * k, d}, x.options().dtype(torch::kFloat32));
  auto out = torch::empty({N, d}, x.options());
  int rc = moe_ffn_bf16(x.data_ptr(), gate_up.data_ptr(), down.data_ptr(),
                        weights.data_ptr<float>(), idx.data_ptr<int>(),
                        sched.data_ptr<int>(), h.data_ptr(),
                        y.data_ptr<float>(), out.data_ptr(), N, (int)d,
                        (int)F, (int)E, (int)k, cur_stream());
  TORCH_CHECK(rc == 0, "moe_ffn: shape not supported by the kernel (N=", N,
              " dim=", d, " ffn_dim=", F, " E=", E, " top_k=", k, ")");
  return out;
}

// x bf16 [M,K]; qweight int32 [N,K/8] or its uint8 view [N,K/2]; scales bf16
// [N,K/128] (format: linear_w4.hip).  splits = 0 takes the kernel's split
// rule; a positive value forces that many K slices (tests and benchmarks
// only — the public op never passes it).  Returns [M,N] bf16.
torch::Tensor linear_w4(torch::Tensor x, torch::Tensor qweight,
                        torch::Tensor scales, int64_t splits) {
  check_bf16(x, "x");
  check_bf16(scales, "scales");
  TORCH_CHECK(qweight.is_cuda() && qweight.is_contiguous() &&
                  (qweight.scalar_type() == torch::kInt32 ||
                   qweight.scalar_type() == torch::kUInt8),
              "linear_w4: qweight must be int32 or uint8, contiguous, on GPU");
  TORCH_CHECK(x.dim() == 2 && qweight.dim() == 2 && scales.dim() == 2,
              "linear_w4: x must be [M,K], qweight [N,K/8], scales [N,K/128]");
  const int64_t per = qweight.scalar_type() == torch::kInt32 ? 8 : 2;
  const int64_t M = x.size(0), K = x.size(1), N = qweight.size(0);
  TORCH_CHECK(M >= 1, "linear_w4: x has no rows");
  TORCH_CHECK(K >= 128 && K % 128 == 0, "linear_w4: K=", K,
              " (must be a multiple of 128)");
  TORCH_CHECK(N >= 64 && N % 64 == 0, "linear_w4: N=", N,
              " (must be a multiple of 64)");
  TORCH_CHECK(qweight.size(1) * per == K && scales.size(0) == N &&
                  scales.size(1) == K / 128,
              "linear_w4: qweight ", qweight.sizes(), " / scales ",
              scales.sizes(), " do not match N=", N, " K=", K);
  TORCH_CHECK(qweight.device() == x.device() && scales.device() == x.device(),
              "linear_w4: all tensors must be on x's device");
  TORCH_CHECK(M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31) &&
                  splits >= 0 && splits < (1ll << 31),
              "linear_w4: size out of range");
  // the kernel reads 16 B fragments
  if ((uintptr_t)x.data_ptr() % 16) x = x.clone();
  if ((uintptr_t)qweight.data_ptr() % 16) qweight = qweight.clone();
  const int S = linear_w4_plan(M, (int)N, (int)K, (int)splits);
  TORCH_CHECK(S >= 1, "linear_w4: shape not supported by the kernel (M=", M,
              " N=", N, " K=", K, " splits=", splits, ")");
  auto out = torch::empty({M, N}, x.options());
  torch::Tensor ws;
  if (S > 1) ws = torch::empty({S, M, N}, x.options().dtype(torch::kFloat32));
  int rc = linear_w4_bf16(x.data_ptr(), qweight.data_ptr(), scales.data_ptr(),
                          S > 1 ? ws.data_ptr<float>() : nullptr,
                          out.data_ptr(), M, (int)N, (int)K, (int)splits,
                          cur_stream());
  TORCH_CHECK(rc == 0, "linear_w4: shape not supported by the kernel (M=", M,
              " N=", N, " K=", K, " splits=", splits, ")");
  return out;
}

int64_t linear_w4_splits(int64_t M, int64_t N, int64_t K, int64_t splits) {
  TORCH_CHECK(M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31) &&
                  splits >= 0 && splits < (1ll << 31),
              "linear_w4: size out of range");
  return linear_w4_plan(M, (int)N, (int)K, (int)splits);
}

torch::Tensor sample_gumbel(torch::Tensor logits, double temperature,
                            int64_t seed) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == torch::kFloat32,
              "logits must be f32 GPU");
  int rows = logits.size(0), V = logits.size(1);
  auto out = torch::empty({rows}, logits.options().dtype(torch::kInt32));
  auto keys = torch::zeros({rows}, logits.options().dtype(torch::kInt64));
  gumbel_sample(logits.data_ptr<float>(),
                (unsigned long long*)keys.data_ptr<int64_t>(),
                out.data_ptr<int>(), rows, V, (float)temperature,
                (unsigned long long)seed, cur_stream());
  return out;
}

// ---- per-row filtered sampling: every parameter is a [rows] device tensor

void check_logits2d(const torch::Tensor& logits) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == torch::kFloat32,
              "logits must be f32 GPU");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(),
              "logits must be [rows, V] contiguous");
  TORCH_CHECK(logits.size(0) > 0 && logits.size(1) > 0 &&
              logits.size(1) < (1ll << 31) && logits.size(0) < (1ll << 22),
              "logits: unsupported shape ", logits.sizes());
}

void check_row_param(const torch::Tensor& t, const torch::Tensor& logits,
                     torch::ScalarType dt, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == logits.device(), name,
              " must be on the logits' GPU");
  TORCH_CHECK(t.scalar_type() == dt, name, " must be ", dt);
  TORCH_CHECK(t.dim() == 1 && t.size(0) == logits.size(0), name,
              " must have one value per row ([", logits.size(0), "]), got ",
              t.sizes());
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

torch::Tensor sampling_cutoff_fwd(torch::Tensor logits, torch::Tensor temps,
                                  torch::Tensor top_k, torch::Tensor top_p,
                                  torch::Tensor min_p) {
  check_logits2d(logits);
  check_row_param(temps, logits, torch::kFloat32, "temperature");
  check_row_param(top_k, logits, torch::kInt32, "top_k");
  check_row_param(top_p, logits, torch::kFloat32, "top_p");
  check_row_param(min_p, logits, torch::kFloat32, "min_p");
  int rows = logits.size(0), V = logits.size(1);
  auto cut = torch::empty({rows}, logits.options());
  sampling_cutoff(logits.data_ptr<float>(), temps.data_ptr<float>(),
                  top_k.data_ptr<int>(), top_p.data_ptr<float>(),
                  min_p.data_ptr<float>(), cut.data_ptr<float>(), rows, V,
                  cur_stream());
  return cut;
}

torch::Tensor sample_batch(torch::Tensor logits, torch::Tensor temps,
                           torch::Tensor seeds, torch::Tensor counters,
                           c10::optional<torch::Tensor> cutoff) {
  check_logits2d(logits);
  check_row_param(temps, logits, torch::kFloat32, "temperature");
  check_row_param(seeds, logits, torch::kInt64, "seeds");
  check_row_param(counters, logits, torch::kInt64, "counters");
  if (cutoff.has_value())
    check_row_param(*cutoff, logits, torch::kFloat32, "cutoff");
  int rows = logits.size(0), V = logits.size(1);
  auto out = torch::empty({rows}, logits.options().dtype(torch::kInt32));
  auto keys = torch::zeros({rows}, logits.options().dtype(torch::kInt64));
  gumbel_sample_batch(
      logits.data_ptr<float>(), temps.data_ptr<float>(),
      (const long long*)seeds.data_ptr<int64_t>(),
      (const long long*)counters.data_ptr<int64_t>(),
      cutoff.has_value() ? cutoff->data_ptr<float>() : nullptr,
      (unsigned long long*)keys.data_ptr<int64_t>(), out.data_ptr<int>(),
      rows, V, cur_stream());
  return out;
}

torch::Tensor softmax_fwd(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kFloat32);
  int V = x.size(-1);
  long long rows = x.numel() / V;
  auto y = torch::empty_like(x);
  softmax_rows(x.data_ptr<float>(), y.data_ptr<float>(), (int)rows, V,
               cur_stream());
  return y;
}

// graph-capturable denoise-step pieces: sigma schedule + step counter live on
// device so one hipGraph capture serves every step.
void scale_in_dev(torch::Tensor x, torch::Tensor y, torch::Tensor sigmas,
                  torch::Tensor step) {
  scale_in_dev_bf16(x.data_ptr(), y.data_ptr(), sigmas.data_ptr<float>(),
                    (const long long*)step.data_ptr<int64_t>(), x.numel(), cur_stream());
}

void cfg_euler_dev(torch::Tensor xt, torch::Tensor eps_c,
                   c10::optional<torch::Tensor> eps_u, torch::Tensor xn,
                   torch::Tensor sigmas, torch::Tensor step, double guidance) {
  cfg_euler_dev_bf16(xt.data_ptr(), eps_c.data_ptr(),
                     eps_u.has_value() ? eps_u->data_ptr() : nullptr,
                     xn.data_ptr(), sigmas.data_ptr<float>(),
                     (const long long*)step.data_ptr<int64_t>(), (float)guidance, xt.numel(),
                     cur_stream());
}

void step_advance(torch::Tensor step) {
  advance_step((long long*)step.data_ptr<int64_t>(), cur_stream());
}

// ---------------------------------------------------------------- snapshot engine
// Pinned-host weight snapshots: one hipHostMalloc region per snapshot, copies
// overlapped across dedicated streams so restore saturates the PCIe Gen5 link
// (the p50-cold-start headline path, BASELINE.json).

struct SnapRegion {
  void* host = nullptr;
  size_t bytes = 0;
  std::vector<hipStream_t> streams;
  size_t rr = 0;
};

std::unordered_map<int64_t, SnapRegion> g_snaps;
int64_t g_next_snap = 1;

int64_t snap_create(int64_t bytes) {
  SnapRegion r;
  r.bytes = (size_t)bytes;
  TORCH_CHECK(hipHostMalloc(&r.host, r.bytes, hipHostMallocDefault) == hipSuccess,
              "hipHostMalloc failed for ", bytes, " bytes");
  r.streams.resize(4);
  for (auto& s : r.streams)
    TORCH_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess);
  int64_t id = g_next_snap++;
  g_snaps[id] = r;
  return id;
}

void snap_save(int64_t id, int64_t offset, torch::Tensor t) {
  auto& r = g_snaps.at(id);
  size_t n = t.numel() * t.element_size();
  TORCH_CHECK((size_t)offset + n <= r.bytes, "snapshot overflow");
  hipStream_t s = r.streams[r.rr++ % r.streams.size()];
  TORCH_CHECK(hipMemcpyAsync((char*)r.host + offset, t.data_ptr(), n,
                             hipMemcpyDeviceToHost, s) == hipSuccess);
}

void snap_restore(int64_t id, int64_t offset, torch::Tensor t) {
  auto& r = g_snaps.at(id);
  size_t n = t.numel() * t.element_size();
  TORCH_CHECK((size_t)offset + n <= r.bytes, "snapshot overflow");
  hipStream_t s = r.streams[r.rr++ % r.streams.size()];
  TORCH_CHECK(hipMemcpyAsync(t.data_ptr(), (char*)r.host + offset, n,
                             hipMemcpyHostToDevice, s) == hipSuccess);
}

void snap_sync(int64_t id) {
  auto& r = g_snaps.at(id);
  for (auto& s : r.streams) TORCH_CHECK(hipStreamSynchronize(s) == hipSuccess);
}

void snap_free(int64_t id) {
  auto it = g_snaps.find(id);
  if (it == g_snaps.end()) return;
  for (auto& s : it->second.streams) hipStreamDestroy(s);
  hipHostFree(it->second.host);
  g_snaps.erase(it);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("attention", &attention, "flash attention fwd bf16 (K1/K5/K7)");
  m.def("attention_bshd", &attention_bshd, "stride-aware attention, BSHD out");
  m.def("attention_fwd_lse", &attention_fwd_lse,
        "attention fwd returning (o, lse) for the backward; out= / lse= "
        "write into the caller's tensors",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("causal"),
        py::arg("scale"), py::arg("out") = py::none(),
        py::arg("lse") = py::none());
  m.def("attention_fwd_lse_bshd", &attention_fwd_lse_bshd,
        "attention fwd returning (o [B,S,H,D], lse); out= / lse= write into "
        "the caller's tensors",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("causal"),
        py::arg("scale"), py::arg("out") = py::none(),
        py::arg("lse") = py::none());
  m.def("attention_bwd", &attention_bwd,
        "flash attention bwd bf16 into caller-provided dq/dk/dv");
  m.def("paged_decode", &paged_decode, "paged KV decode attention (K6)");
  m.def("paged_prefill", &paged_prefill,
        "paged KV prefill attention: ragged causal chunks over a cached "
        "prefix (K6)");
  m.def("groupnorm_silu", &groupnorm_silu);
  m.def("groupnorm_silu_nhwc", &groupnorm_silu_nhwc,
        "GroupNorm(+SiLU) of NCHW x, written as [N, H*W, C]");
  m.def("layernorm", &layernorm);
  m.def("add_layernorm", &add_layernorm,
        "(x + y, LayerNorm(x + y)) from one read of x and y");
  m.def("add_nhwc_to_nchw", &add_nhwc_to_nchw,
        "res [N,C,H,W] + h [N,H*W,C], tiled transpose in LDS");
  m.def("scaled_softmax", &scaled_softmax,
        "softmax((s * scale).float(), -1).to(bf16), bf16 in and out");
  m.def("rmsnorm", &rmsnorm);
  m.def("cfg_euler", &cfg_euler, "fused CFG + Euler step (K4)");
  m.def("silu_mul", &silu_mul);
  m.def("geglu", &geglu);
  m.def("glu_fused", &glu_fused, "in-place-sliced silu/gelu-mul over a fused [.,2I] projection");
  m.def("add_residual", &add_residual);
  m.def("rope_", &rope_, "in-place RoPE with host cos/sin tables");
  m.def("adamw_", &adamw_, "fused AdamW step (K9)");
  m.def("sample_gumbel", &sample_gumbel, "fused sampling (K8)");
  m.def("sample_batch", &sample_batch,
        "per-row temperature/seed/counter/cutoff gumbel sampling (K8)");
  m.def("sampling_cutoff", &sampling_cutoff_fwd,
        "per-row top-k/top-p/min-p logit cutoff by radix select (K8)");
  m.def("conv3x3", &conv3x3,
        "NCHW implicit-GEMM 3x3 conv, fused bias + residual or [N,K] addend "
        "(K3)",
        pybind11::arg("x"), pybind11::arg("wr"), pybind11::arg("bias"),
        pybind11::arg("residual"), pybind11::arg("K"),
        pybind11::arg("upsample"), pybind11::arg("addend") = pybind11::none());
  m.def("conv3x3_gn", &conv3x3_gn, "GroupNorm+SiLU fused into the K3 conv");
  m.def("softmax_fwd", &softmax_fwd);
  m.def("moe_route", &moe_route,
        "MoE top-k routing: (weights fp32 [N,k], idx int32 [N,k])");
  m.def("moe_ffn", &moe_ffn,
        "fused MoE FFN: on-device schedule, grouped MFMA GEMMs, combine");
  m.def("linear_w4", &linear_w4,
        "int4 weight-only linear: in-register dequant, MFMA, split-K",
        pybind11::arg("x"), pybind11::arg("qweight"), pybind11::arg("scales"),
        pybind11::arg("splits") = 0);
  m.def("linear_w4_splits", &linear_w4_splits,
        "K slices linear_w4 uses for (M, N, K); 0 = unsupported shape",
        pybind11::arg("M"), pybind11::arg("N"), pybind11::arg("K"),
        pybind11::arg("splits") = 0);
  m.def("scale_in_dev", &scale_in_dev, "x * 1/sqrt(sigma^2+1), device sigma");
  m.def("cfg_euler_dev", &cfg_euler_dev, "graph-capturable CFG+Euler step");
  m.def("step_advance", &step_advance, "increment device step counter");
  m.def("snap_create", &snap_create, "pinned-host snapshot region (K13)");
  m.def("snap_save", &snap_save);
  m.def("snap_restore", &snap_restore);
  m.def("snap_sync", &snap_sync);
  m.def("snap_free", &snap_free);
}
