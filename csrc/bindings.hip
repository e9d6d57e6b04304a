// Torch extension bindings for the MI355X kernels.
//
// All entry points take torch tensors on the current CUDA(HIP) device and
// launch on the current stream. u64 masks travel as int64 tensors
// (bitwise-identical).
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <vector>

#define CHECK_GPU(x) TORCH_CHECK(x.is_cuda(), #x " must be on GPU")
#define CHECK_CONTIG(x) TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")

extern "C" {
__global__ void sha256_leaves_kernel(const uint8_t*, const int32_t*, uint8_t*, int);
__global__ void merkle_level_kernel(const uint8_t*, uint8_t*, int);
__global__ void dfa_scan_kernel(const uint8_t*, const int32_t*, const uint16_t*,
                                const unsigned long long*, const unsigned long long*,
                                const uint8_t*, const int32_t*, int,
                                unsigned long long*, int);
__global__ void encode_messages_kernel(const uint8_t*, const int32_t*, const __bf16*,
                                       int, int, __bf16*, int, int);
__global__ void gemm_nt_bf16_kernel(const __bf16*, const __bf16*, float*, __bf16*,
                                    const float*, int, int, int, int, int);
__global__ void topk_recall_kernel(const __bf16*, const __bf16*, int, int, int, int,
                                   int, float*, int32_t*, const float*, int32_t*, int,
                                   const int32_t*, const int32_t*);
__global__ void topk_recall_fp8_kernel(const uint8_t*, const uint8_t*, int, int, int,
                                       int, int, float*, int32_t*, const float*,
                                       int32_t*, int);
__global__ void topk_scan_mx_kernel(const uint8_t*, const uint8_t*, int, int, int,
                                    int, int, float*, int32_t*, const float*,
                                    int32_t*, int);
__global__ void topk_scan_mx4_kernel(const uint8_t*, const uint8_t*, const uint8_t*,
                                     int, int, int, int, int, float*, int32_t*,
                                     const float*, int32_t*, int);
__global__ void topk_scan_fp4_kernel(const uint8_t*, const uint8_t*, const uint8_t*,
                                     const uint8_t*, int, int, int, int, int,
                                     float*, int32_t*, const float*, int32_t*, int);
__global__ void topk_scan_fp4_v2_kernel(const uint8_t*, const uint8_t*, const uint8_t*,
                                        const uint8_t*, int, int, int, int, int,
                                        float*, int32_t*, const float*, int32_t*, int);
__global__ void topk_scan_fp4_v3_kernel(const uint8_t*, const uint8_t*, const uint8_t*,
                                        const uint8_t*, int, int, int, int, int,
                                        float*, int32_t*, const float*, int32_t*, int);
__global__ void topk_scan_fp4_v5_kernel(const uint8_t*, const uint8_t*, const uint8_t*,
                                        const uint8_t*, int, int, int, int, int,
                                        float*, int32_t*, const float*, int32_t*, int);
__global__ void topk_scan_fp4_v7_kernel(const uint8_t*, const uint8_t*, const uint8_t*,
                                        const uint8_t*, int, int, int, int, int,
                                        float*, int32_t*, const float*, int32_t*, int);
__global__ void topk_scan_fp4_v9_kernel(const uint8_t*, const uint8_t*, const uint8_t*,
                                        const uint8_t*, int, int, int, int, int,
                                        float*, int32_t*, const float*, int32_t*, int);
__global__ void topk_scan_fp4_v10_kernel(const uint8_t*, const uint8_t*, const uint8_t*,
                                         const uint8_t*, int, int, int, int, int,
                                         float*, int32_t*, const float*, int32_t*, int);
__global__ void topk_scan_fp4_owned_kernel(const uint8_t*, const uint8_t*, const uint8_t*,
                                           const uint8_t*, int, int, int, int, int,
                                           float*, int32_t*, const float*, int32_t*, int,
                                           const int32_t*, const int32_t*);
__global__ void topk_scan_fp4_hist_kernel(const uint8_t*, const uint8_t*, const uint8_t*,
                                          const uint8_t*, int, int, int, int, int,
                                          float*, int32_t*, const float*, int32_t*, int,
                                          int32_t*, const float*, const float*);
__global__ void topk_scan_fp4_owned_hist_kernel(const uint8_t*, const uint8_t*,
                                                const uint8_t*, const uint8_t*, int, int,
                                                int, int, int, float*, int32_t*,
                                                const float*, int32_t*, int,
                                                const int32_t*, const int32_t*,
                                                int32_t*, const float*, const float*);

__global__ void topk_merge_kernel(const float*, const int32_t*, int, int, int,
                                  float*, int32_t*);
__global__ void firewall_verdict_kernel(const unsigned long long*, const unsigned long long*,
                                        const float*, int, const int32_t*, const float*,
                                        const float*, const int32_t*, int,
                                        unsigned long long, float, int8_t*, float*,
                                        float*, float*, int);
__global__ void trust_recompute_kernel(float*, float*, const float*, const float*,
                                       const float*, float*, const float*, float*, int);
__global__ void edit_distance_kernel(const uint8_t*, const int32_t*, int32_t*, int);
__global__ void dfa_scan_multi_kernel(const uint8_t*, const int32_t*, const uint16_t*,
                                      const unsigned long long*, const unsigned long long*,
                                      const uint8_t*, const int32_t*, const int32_t*,
                                      int, unsigned long long*, int, int);
__global__ void fact_probe_kernel(const uint8_t*, const int32_t*,
                                  const unsigned long long*, const unsigned long long*,
                                  const unsigned long long*, const unsigned long long*,
                                  int, int32_t*, int32_t*, int);
__global__ void fp4_quantize_append_kernel(const uint16_t*, const int32_t*, int, long long,
                                           int, long long, uint16_t*, uint8_t*, uint8_t*,
                                           int32_t*, const int32_t*, float*, float,
                                           long long*, long long);
__global__ void index_move_rows_kernel(const int32_t*, const int32_t*, long long, int, int,
                                       uint4*, uint4*, uint32_t*, uint32_t*, uint32_t*,
                                       uint2*);
__global__ void index_find_ids_kernel(const long long*, long long, const long long*, int,
                                      int32_t*);
__global__ void batch_first_similar_kernel(const __bf16*, const uint8_t*, const int32_t*,
                                           int, int, float, int32_t*);
__global__ void recall_dup_rows_kernel(const uint4*, const int32_t*, const uint4*,
                                       const int32_t*, const int32_t*, int, int, int, int,
                                       float, int32_t*, float*);
__global__ void row_moments_kernel(const uint16_t*, int, float*, float*);
__global__ void select_rescore_kernel(const float*, const int32_t*, const int32_t*,
                                      const uint4*, const uint4*, const float*, int, int,
                                      int, int, int, float*, int32_t*);
struct AuditRecord64;
__global__ void audit_pack_kernel(const int8_t*, const float*, const unsigned long long*,
                                  const unsigned long long*, const int32_t*, const float*,
                                  const float*, long long, long long, uint32_t,
                                  AuditRecord64*, int);
}

static hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

torch::Tensor sha256_leaves(torch::Tensor bytes, torch::Tensor offsets) {
  CHECK_GPU(bytes); CHECK_CONTIG(bytes); CHECK_GPU(offsets); CHECK_CONTIG(offsets);
  TORCH_CHECK(bytes.dtype() == torch::kUInt8 && offsets.dtype() == torch::kInt32);
  int n = offsets.numel() - 1;
  auto out = torch::empty({n, 32}, bytes.options());
  int threads = 128;
  int blocks = (n + threads - 1) / threads;
  hipLaunchKernelGGL(sha256_leaves_kernel, dim3(blocks), dim3(threads), 0, cur_stream(),
                     bytes.data_ptr<uint8_t>(), offsets.data_ptr<int32_t>(),
                     out.data_ptr<uint8_t>(), n);
  return out;
}

torch::Tensor merkle_root_gpu(torch::Tensor digests) {
  CHECK_GPU(digests); CHECK_CONTIG(digests);
  TORCH_CHECK(digests.dtype() == torch::kUInt8 && digests.size(1) == 32);
  int n = digests.size(0);
  TORCH_CHECK(n >= 1);
  auto cur = digests;
  while (n > 1) {
    int n_out = (n + 1) / 2;
    auto nxt = torch::empty({n_out, 32}, digests.options());
    int threads = 128;
    int blocks = (n_out + threads - 1) / threads;
    hipLaunchKernelGGL(merkle_level_kernel, dim3(blocks), dim3(threads), 0, cur_stream(),
                       cur.data_ptr<uint8_t>(), nxt.data_ptr<uint8_t>(), n);
    cur = nxt;
    n = n_out;
  }
  return cur.reshape({32});
}

torch::Tensor dfa_scan(torch::Tensor bytes, torch::Tensor offsets, torch::Tensor next_tab,
                       torch::Tensor accept, torch::Tensor eof_mask,
                       torch::Tensor class_maps, torch::Tensor meta) {
  CHECK_GPU(bytes); CHECK_GPU(offsets); CHECK_GPU(next_tab); CHECK_GPU(accept);
  CHECK_GPU(eof_mask); CHECK_GPU(class_maps); CHECK_GPU(meta);
  TORCH_CHECK(next_tab.dtype() == torch::kInt16 || next_tab.dtype() == torch::kUInt8 ||
              next_tab.scalar_type() == at::kShort, "next_tab must be int16 view of u16");
  int n = offsets.numel() - 1;
  int n_dfas = meta.size(0);
  auto hits = torch::zeros({n}, torch::dtype(torch::kInt64).device(bytes.device()));
  int threads = 256;
  int blocks = (n + threads - 1) / threads;
  size_t lds = (size_t)n_dfas * 256;
  hipLaunchKernelGGL(dfa_scan_kernel, dim3(blocks), dim3(threads), lds, cur_stream(),
                     bytes.data_ptr<uint8_t>(), offsets.data_ptr<int32_t>(),
                     reinterpret_cast<const uint16_t*>(next_tab.data_ptr()),
                     reinterpret_cast<const unsigned long long*>(accept.data_ptr<int64_t>()),
                     reinterpret_cast<const unsigned long long*>(eof_mask.data_ptr<int64_t>()),
                     class_maps.data_ptr<uint8_t>(), meta.data_ptr<int32_t>(), n_dfas,
                     reinterpret_cast<unsigned long long*>(hits.data_ptr<int64_t>()), n);
  return hits;
}

// One launch scanning ALL families: family_ranges [n_families, 2] rows of
// (begin, end) into meta rows; hits come back as int64 [n_families, n].
torch::Tensor dfa_scan_multi(torch::Tensor bytes, torch::Tensor offsets,
                             torch::Tensor next_tab, torch::Tensor accept,
                             torch::Tensor eof_mask, torch::Tensor class_maps,
                             torch::Tensor meta, torch::Tensor family_ranges) {
  CHECK_GPU(bytes); CHECK_GPU(offsets); CHECK_GPU(next_tab); CHECK_GPU(accept);
  CHECK_GPU(eof_mask); CHECK_GPU(class_maps); CHECK_GPU(meta); CHECK_GPU(family_ranges);
  int n = offsets.numel() - 1;
  int n_dfas = meta.size(0);
  int n_families = family_ranges.size(0);
  CHECK_CONTIG(bytes); CHECK_CONTIG(offsets); CHECK_CONTIG(meta); CHECK_CONTIG(family_ranges);
  TORCH_CHECK(bytes.numel() <= INT32_MAX, "dfa_scan_multi: offsets are int32");
  auto hits = torch::zeros({n_families, n},
                           torch::dtype(torch::kInt64).device(bytes.device()));
  if (n <= 0 || n_dfas <= 0) return hits;
  TORCH_CHECK(n_dfas <= 65535, "dfa_scan_multi: too many sub-DFAs for grid.y");
  // grid = messages x sub-DFAs; 128 = DFA_MULTI_THREADS (csrc/pattern_scan.hip):
  // two-wave blocks spread the 1792 waves of a 4096-message batch over all CUs
  int threads = 128;
  int blocks = (n + threads - 1) / threads;
  hipLaunchKernelGGL(dfa_scan_multi_kernel, dim3(blocks, n_dfas), dim3(threads), 0, cur_stream(),
                     bytes.data_ptr<uint8_t>(), offsets.data_ptr<int32_t>(),
                     reinterpret_cast<const uint16_t*>(next_tab.data_ptr()),
                     reinterpret_cast<const unsigned long long*>(accept.data_ptr<int64_t>()),
                     reinterpret_cast<const unsigned long long*>(eof_mask.data_ptr<int64_t>()),
                     class_maps.data_ptr<uint8_t>(), meta.data_ptr<int32_t>(),
                     family_ranges.data_ptr<int32_t>(), n_families,
                     reinterpret_cast<unsigned long long*>(hits.data_ptr<int64_t>()),
                     n, (int)bytes.numel());
  return hits;
}

// GPU fact-registry probe (csrc/fact_probe.hip): returns per-message
// (verified, contradicted) counts for claim-bearing messages.
std::vector<torch::Tensor> fact_probe(torch::Tensor bytes, torch::Tensor offsets,
                                      torch::Tensor claims_mask, torch::Tensor pred_hash,
                                      torch::Tensor table_keys, torch::Tensor table_vals,
                                      int64_t table_pow2) {
  CHECK_GPU(bytes); CHECK_GPU(offsets); CHECK_GPU(claims_mask);
  CHECK_GPU(pred_hash); CHECK_GPU(table_keys); CHECK_GPU(table_vals);
  TORCH_CHECK(pred_hash.numel() == 64, "pred_hash must have 64 entries");
  TORCH_CHECK(table_keys.numel() == (1ll << table_pow2), "table size mismatch");
  int n = offsets.numel() - 1;
  auto opts = torch::dtype(torch::kInt32).device(bytes.device());
  auto verified = torch::zeros({n}, opts);
  auto contradicted = torch::zeros({n}, opts);
  int threads = 256;
  int blocks = (n + threads - 1) / threads;
  hipLaunchKernelGGL(fact_probe_kernel, dim3(blocks), dim3(threads), 0, cur_stream(),
                     bytes.data_ptr<uint8_t>(), offsets.data_ptr<int32_t>(),
                     reinterpret_cast<const unsigned long long*>(claims_mask.data_ptr<int64_t>()),
                     reinterpret_cast<const unsigned long long*>(pred_hash.data_ptr<int64_t>()),
                     reinterpret_cast<const unsigned long long*>(table_keys.data_ptr<int64_t>()),
                     reinterpret_cast<const unsigned long long*>(table_vals.data_ptr<int64_t>()),
                     (int)table_pow2, verified.data_ptr<int32_t>(),
                     contradicted.data_ptr<int32_t>(), n);
  return {verified, contradicted};
}

torch::Tensor encode_messages(torch::Tensor bytes, torch::Tensor offsets,
                              torch::Tensor embed, bool normalize) {
  CHECK_GPU(bytes); CHECK_GPU(offsets); CHECK_GPU(embed); CHECK_CONTIG(embed);
  TORCH_CHECK(embed.dtype() == torch::kBFloat16);
  int vocab = embed.size(0);
  int dim = embed.size(1);
  TORCH_CHECK((vocab & (vocab - 1)) == 0, "vocab must be a power of two");
  // the kernel walks 1024-dim chunks (256 threads x 4 dims) and guards the
  // tail of a single short chunk
  TORCH_CHECK(dim % 1024 == 0 || (dim < 1024 && dim % 4 == 0),
              "dim must be a multiple of 1024, or a multiple of 4 below 1024");
  int n = offsets.numel() - 1;
  auto out = torch::empty({n, dim}, embed.options());
  hipLaunchKernelGGL(encode_messages_kernel, dim3(n), dim3(256), 0, cur_stream(),
                     bytes.data_ptr<uint8_t>(), offsets.data_ptr<int32_t>(),
                     reinterpret_cast<const __bf16*>(embed.data_ptr()), vocab - 1, dim,
                     reinterpret_cast<__bf16*>(out.data_ptr()), n, normalize ? 1 : 0);
  return out;
}

torch::Tensor gemm_nt(torch::Tensor A, torch::Tensor B,
                      c10::optional<torch::Tensor> bias, int64_t act, bool out_bf16) {
  CHECK_GPU(A); CHECK_CONTIG(A); CHECK_GPU(B); CHECK_CONTIG(B);
  TORCH_CHECK(A.dtype() == torch::kBFloat16 && B.dtype() == torch::kBFloat16);
  int M = A.size(0), K = A.size(1), N = B.size(0);
  TORCH_CHECK(B.size(1) == K, "K mismatch");
  TORCH_CHECK(K % 32 == 0, "K must be a multiple of 32");
  auto opts = torch::dtype(out_bf16 ? torch::kBFloat16 : torch::kFloat32).device(A.device());
  auto C = torch::empty({M, N}, opts);
  const float* bias_ptr = nullptr;
  if (bias.has_value()) {
    CHECK_GPU(bias.value());
    TORCH_CHECK(bias->dtype() == torch::kFloat32 && bias->numel() == N);
    bias_ptr = bias->data_ptr<float>();
  }
  dim3 grid((M + 127) / 128, (N + 127) / 128);
  hipLaunchKernelGGL(gemm_nt_bf16_kernel, grid, dim3(256), 0, cur_stream(),
                     reinterpret_cast<const __bf16*>(A.data_ptr()),
                     reinterpret_cast<const __bf16*>(B.data_ptr()),
                     out_bf16 ? nullptr : C.data_ptr<float>(),
                     out_bf16 ? reinterpret_cast<__bf16*>(C.data_ptr()) : nullptr,
                     bias_ptr, M, N, K, (int)act, out_bf16 ? 1 : 0);
  return C;
}

// Owner filter operands: xowner int32 [nx] (values >= 0), qowner int32
// [nq] (< 0 = unfiltered). Both or neither.
static void check_owners(const torch::Tensor& xowner, const torch::Tensor& qowner,
                         long long nx, long long nq) {
  CHECK_GPU(xowner); CHECK_CONTIG(xowner); CHECK_GPU(qowner); CHECK_CONTIG(qowner);
  TORCH_CHECK(xowner.dtype() == torch::kInt32 && qowner.dtype() == torch::kInt32,
              "xowner and qowner must be int32");
  TORCH_CHECK(xowner.dim() == 1 && xowner.numel() == nx,
              "xowner must have one entry per index row");
  TORCH_CHECK(qowner.dim() == 1 && qowner.numel() == nq,
              "qowner must have one entry per query");
}

static bool have_owners(const c10::optional<torch::Tensor>& xowner,
                        const c10::optional<torch::Tensor>& qowner,
                        long long nx, long long nq) {
  TORCH_CHECK(xowner.has_value() == qowner.has_value(),
              "xowner and qowner must be given together");
  if (!xowner.has_value()) return false;
  check_owners(*xowner, *qowner, nx, nq);
  return true;
}

std::vector<torch::Tensor> topk_recall(torch::Tensor Q, torch::Tensor X, int64_t k,
                                       int64_t n_swaths,
                                       c10::optional<torch::Tensor> xowner,
                                       c10::optional<torch::Tensor> qowner) {
  CHECK_GPU(Q); CHECK_CONTIG(Q); CHECK_GPU(X); CHECK_CONTIG(X);
  TORCH_CHECK(Q.dtype() == torch::kBFloat16 && X.dtype() == torch::kBFloat16);
  int nq = Q.size(0), D = Q.size(1);
  long long nx = X.size(0);
  bool owned = have_owners(xowner, qowner, nx, nq);
  TORCH_CHECK(X.size(1) == D && D % 64 == 0, "D must be a multiple of 64");
  TORCH_CHECK(k >= 1 && k <= 32, "k in [1,32]");
  int n_qblocks = (nq + 255) / 256;  // BM=256 (topk_recall.hip v3)
  // merge kernel holds n_swaths*k candidates in 16 regs x 64 lanes
  TORCH_CHECK(n_swaths >= 1 && (long long)n_swaths * k <= 1024,
              "n_swaths * k must be <= 1024");
  auto f32opts = torch::dtype(torch::kFloat32).device(Q.device());
  auto i32opts = torch::dtype(torch::kInt32).device(Q.device());
  // candidate state lives in global memory, host-initialized; the kernel
  // only updates slots that beat the running per-row threshold
  auto cand_s = torch::full({(long long)n_qblocks * n_swaths * 256 * k}, -1e30,
                            f32opts);
  auto cand_i = torch::full({(long long)n_qblocks * n_swaths * 256 * k}, -1,
                            i32opts);
  // flat grid: block f -> (qb = f / S, swath = f % S); S a multiple of 8
  // keeps each co-sweeping same-swath group on one XCD
  dim3 grid((unsigned)(n_qblocks * n_swaths));
  // 512 threads = the kernel's 8-wave 2x4 grid (TK_THREADS in topk_recall.hip)
  hipLaunchKernelGGL(topk_recall_kernel, grid, dim3(512), 0, cur_stream(),
                     reinterpret_cast<const __bf16*>(Q.data_ptr()),
                     reinterpret_cast<const __bf16*>(X.data_ptr()), nq, (int)nx, D,
                     (int)k, (int)n_swaths, cand_s.data_ptr<float>(),
                     cand_i.data_ptr<int32_t>(), nullptr, nullptr, 0,
                     owned ? xowner->data_ptr<int32_t>() : nullptr,
                     owned ? qowner->data_ptr<int32_t>() : nullptr);
  auto out_s = torch::empty({nq, k}, f32opts);
  auto out_i = torch::empty({nq, k}, i32opts);
  int waves_per_block = 4;
  int blocks = (nq + waves_per_block - 1) / waves_per_block;
  hipLaunchKernelGGL(topk_merge_kernel, dim3(blocks), dim3(waves_per_block * 64), 0,
                     cur_stream(), cand_s.data_ptr<float>(), cand_i.data_ptr<int32_t>(),
                     nq, (int)k, (int)n_swaths, out_s.data_ptr<float>(),
                     out_i.data_ptr<int32_t>());
  return {out_s, out_i};
}

std::vector<torch::Tensor> topk_recall_fp8(torch::Tensor Q8, torch::Tensor X8,
                                           int64_t k, int64_t n_swaths) {
  // stage-1 fp8 scan of the two-stage recall: inputs are e4m3 bytes
  // (viewed as uint8), pre-scaled x8; scores rank candidates only.
  CHECK_GPU(Q8); CHECK_CONTIG(Q8); CHECK_GPU(X8); CHECK_CONTIG(X8);
  TORCH_CHECK(Q8.dtype() == torch::kUInt8 && X8.dtype() == torch::kUInt8,
              "fp8 operands passed as uint8 views");
  int nq = Q8.size(0), D = Q8.size(1);
  long long nx = X8.size(0);
  TORCH_CHECK(X8.size(1) == D && D % 64 == 0, "D must be a multiple of 64");
  TORCH_CHECK(k >= 1 && k <= 32, "k in [1,32]");  // TOPK_MAX LDS bound
  int n_qblocks = (nq + 255) / 256;
  TORCH_CHECK(n_swaths >= 1 && (long long)n_swaths * k <= 1024,
              "n_swaths * k must be <= 1024");
  auto f32opts = torch::dtype(torch::kFloat32).device(Q8.device());
  auto i32opts = torch::dtype(torch::kInt32).device(Q8.device());
  auto cand_s = torch::full({(long long)n_qblocks * n_swaths * 256 * k}, -1e30,
                            f32opts);
  auto cand_i = torch::full({(long long)n_qblocks * n_swaths * 256 * k}, -1,
                            i32opts);
  dim3 grid((unsigned)(n_qblocks * n_swaths));
  hipLaunchKernelGGL(topk_recall_fp8_kernel, grid, dim3(512), 0, cur_stream(),
                     Q8.data_ptr<uint8_t>(), X8.data_ptr<uint8_t>(), nq, (int)nx,
                     D, (int)k, (int)n_swaths, cand_s.data_ptr<float>(),
                     cand_i.data_ptr<int32_t>(), nullptr, nullptr, 0);
  auto out_s = torch::empty({nq, k}, f32opts);
  auto out_i = torch::empty({nq, k}, i32opts);
  int waves_per_block = 4;
  int blocks = (nq + waves_per_block - 1) / waves_per_block;
  hipLaunchKernelGGL(topk_merge_kernel, dim3(blocks), dim3(waves_per_block * 64), 0,
                     cur_stream(), cand_s.data_ptr<float>(), cand_i.data_ptr<int32_t>(),
                     nq, (int)k, (int)n_swaths, out_s.data_ptr<float>(),
                     out_i.data_ptr<int32_t>());
  return {out_s, out_i};
}

std::vector<torch::Tensor> firewall_verdict(
    torch::Tensor inj_hits, torch::Tensor red_hits, torch::Tensor logits,
    torch::Tensor agent_idx, torch::Tensor agent_trust, torch::Tensor tool_risk,
    torch::Tensor freq_count, int64_t hour, int64_t cred_bits, double inj_threshold,
    int64_t n_agents) {
  CHECK_GPU(inj_hits); CHECK_GPU(red_hits); CHECK_GPU(logits); CHECK_GPU(agent_idx);
  CHECK_GPU(agent_trust); CHECK_GPU(tool_risk); CHECK_GPU(freq_count);
  int B = inj_hits.numel();
  int n_cls = logits.size(1);
  auto verdict = torch::empty({B}, torch::dtype(torch::kInt8).device(inj_hits.device()));
  auto risk = torch::empty({B}, torch::dtype(torch::kFloat32).device(inj_hits.device()));
  auto sdelta = torch::zeros({n_agents}, torch::dtype(torch::kFloat32).device(inj_hits.device()));
  auto vdelta = torch::zeros({n_agents}, torch::dtype(torch::kFloat32).device(inj_hits.device()));
  int threads = 256;
  int blocks = (B + threads - 1) / threads;
  hipLaunchKernelGGL(firewall_verdict_kernel, dim3(blocks), dim3(threads), 0, cur_stream(),
                     reinterpret_cast<const unsigned long long*>(inj_hits.data_ptr<int64_t>()),
                     reinterpret_cast<const unsigned long long*>(red_hits.data_ptr<int64_t>()),
                     logits.data_ptr<float>(), n_cls, agent_idx.data_ptr<int32_t>(),
                     agent_trust.data_ptr<float>(), tool_risk.data_ptr<float>(),
                     freq_count.data_ptr<int32_t>(), (int)hour,
                     (unsigned long long)cred_bits, (float)inj_threshold,
                     verdict.data_ptr<int8_t>(), risk.data_ptr<float>(),
                     sdelta.data_ptr<float>(), vdelta.data_ptr<float>(), B);
  return {verdict, risk, sdelta, vdelta};
}

void trust_recompute(torch::Tensor success_count, torch::Tensor violation_count,
                     torch::Tensor success_delta, torch::Tensor violation_delta,
                     torch::Tensor age_days, torch::Tensor clean_streak,
                     torch::Tensor manual_adj, torch::Tensor score) {
  int A = score.numel();
  int threads = 256;
  int blocks = (A + threads - 1) / threads;
  hipLaunchKernelGGL(trust_recompute_kernel, dim3(blocks), dim3(threads), 0, cur_stream(),
                     success_count.data_ptr<float>(), violation_count.data_ptr<float>(),
                     success_delta.data_ptr<float>(), violation_delta.data_ptr<float>(),
                     age_days.data_ptr<float>(), clean_streak.data_ptr<float>(),
                     manual_adj.data_ptr<float>(), score.data_ptr<float>(), A);
}

torch::Tensor audit_pack(torch::Tensor verdict, torch::Tensor risk, torch::Tensor inj_hits,
                         torch::Tensor red_hits, torch::Tensor agent_idx,
                         torch::Tensor agent_trust, torch::Tensor inj_score,
                         int64_t ts_ms, int64_t msg_id0, int64_t batch_seq) {
  int B = verdict.numel();
  auto out = torch::empty({B, 64}, torch::dtype(torch::kUInt8).device(verdict.device()));
  int threads = 256;
  int blocks = (B + threads - 1) / threads;
  hipLaunchKernelGGL(audit_pack_kernel, dim3(blocks), dim3(threads), 0, cur_stream(),
                     verdict.data_ptr<int8_t>(), risk.data_ptr<float>(),
                     reinterpret_cast<const unsigned long long*>(inj_hits.data_ptr<int64_t>()),
                     reinterpret_cast<const unsigned long long*>(red_hits.data_ptr<int64_t>()),
                     agent_idx.data_ptr<int32_t>(), agent_trust.data_ptr<float>(),
                     inj_score.data_ptr<float>(), (long long)ts_ms, (long long)msg_id0,
                     (uint32_t)batch_seq,
                     reinterpret_cast<AuditRecord64*>(out.data_ptr<uint8_t>()), B);
  return out;
}


// Shared body of the unfiltered and the owner-filtered fp4x4 bindings:
// same operand checks, swath heuristic and candidate buffers. With owners
// the launch is topk_scan_fp4_owned_kernel and variant_arg is unused.
static std::vector<torch::Tensor> fp4x4_scan(
    torch::Tensor Q4, torch::Tensor QS, torch::Tensor X4, torch::Tensor XS,
    torch::Tensor theta, int64_t cap, int64_t n_swaths, int64_t variant_arg,
    bool scan_only, const torch::Tensor* xowner, const torch::Tensor* qowner,
    const torch::Tensor* hist_w = nullptr) {
  // both operands MXFP4 (csrc topk_scan_fp4_kernel); scores at x1.
  // variant_arg: -1 = environment/default, 0 = v1, 1 = v2, 2 = v3,
  // 4 = v5, 7 = v7, 9 = v9, 10 = v10. scan_only runs the K-loops without
  // the epilogue (k = -1) for epilogue-share attribution.
  CHECK_GPU(Q4); CHECK_CONTIG(Q4); CHECK_GPU(QS); CHECK_CONTIG(QS);
  CHECK_GPU(X4); CHECK_CONTIG(X4); CHECK_GPU(XS); CHECK_CONTIG(XS);
  CHECK_GPU(theta); CHECK_CONTIG(theta);
  int nq = Q4.size(0), D = (int)Q4.size(1) * 2;
  long long nx = X4.size(0);
  TORCH_CHECK(D % 128 == 0 && D / 32 <= 32, "fp4x4 kernel caps at D=1024");
  TORCH_CHECK(QS.size(0) == nq && QS.size(1) == D / 32);
  TORCH_CHECK(X4.size(1) == D / 2 && XS.size(0) == nx && XS.size(1) == D / 32);
  TORCH_CHECK(theta.numel() == nq && cap >= 32 && cap <= 4096);
  if (xowner != nullptr) check_owners(*xowner, *qowner, nx, nq);
  // v10 (v9 = v7 + transposed scale sheets read as one dword per fragment
  // per four pairs with the byte picked by op_sel, counted lgkmcnt per m;
  // v10 = v9 on the fragment swizzle that is conflict-free on the real
  // ds_read_b128 lane groups) is the default: bit-exact vs v1, and every
  // bench run below every v9 run, 109.7 vs 114.8 ms/step (profiles/README).
  // Env overrides for A/B; VAINPLEX_FP4_V9=1 is the way back to v9.
  static const int env_variant = [] {
    if (const char* e = getenv("VAINPLEX_FP4_V1"); e && e[0] == '1') return 0;
    if (const char* e = getenv("VAINPLEX_FP4_V2"); e && e[0] == '1') return 1;
    if (const char* e = getenv("VAINPLEX_FP4_V3"); e && e[0] == '1') return 2;
    if (const char* e = getenv("VAINPLEX_FP4_V5"); e && e[0] == '1') return 4;
    if (const char* e = getenv("VAINPLEX_FP4_V7"); e && e[0] == '1') return 7;
    if (const char* e = getenv("VAINPLEX_FP4_V9"); e && e[0] == '1') return 9;
    return 10;
  }();
  int variant = variant_arg < 0 ? env_variant : (int)variant_arg;
  TORCH_CHECK(variant == 0 || variant == 1 || variant == 2 || variant == 4 ||
              variant == 7 || variant == 9 || variant == 10,
              "fp4x4 scan: unknown variant ", variant);
  int n_qblocks = (nq + 255) / 256;
  if (n_swaths <= 0) {
    int want = 256 / (n_qblocks > 0 ? n_qblocks : 1);
    n_swaths = want >= 8 ? (want / 8) * 8 : 8;
    long long max_s = nx / 256; if (max_s < 1) max_s = 1;
    if (n_swaths > max_s) n_swaths = max_s;
  }
  auto f32opts = torch::dtype(torch::kFloat32).device(Q4.device());
  auto i32opts = torch::dtype(torch::kInt32).device(Q4.device());
  auto cand_s = torch::full({(long long)nq, cap}, -1e30, f32opts);
  auto cand_i = torch::full({(long long)nq, cap}, -1, i32opts);
  auto counts = torch::zeros({(long long)nq}, i32opts);
  dim3 grid((unsigned)(n_qblocks * n_swaths));
  if (hist_w != nullptr) {
    // v10 / owned scan that also counts, by score bin, the hits that found
    // the buffer full: bins of width hist_w[q] above theta[q] (csrc
    // topk_scan_fp4_hist_kernel, ops.gpu.hist_bin_spec)
    const torch::Tensor& w = *hist_w;
    CHECK_GPU(w); CHECK_CONTIG(w);
    TORCH_CHECK(theta.dtype() == torch::kFloat32 && w.dtype() == torch::kFloat32,
                "theta and w must be float32");
    TORCH_CHECK(w.dim() == 1 && w.numel() == nq, "w must have one entry per query");
    auto inv_w = w.reciprocal();
    auto hist = torch::zeros({(long long)nq, 256}, i32opts);
    if (xowner != nullptr)
      hipLaunchKernelGGL(topk_scan_fp4_owned_hist_kernel, grid, dim3(512), 0,
                         cur_stream(),
                         Q4.data_ptr<uint8_t>(), QS.data_ptr<uint8_t>(),
                         X4.data_ptr<uint8_t>(), XS.data_ptr<uint8_t>(),
                         nq, (int)nx, D, 1, (int)n_swaths,
                         cand_s.data_ptr<float>(), cand_i.data_ptr<int32_t>(),
                         theta.data_ptr<float>(), counts.data_ptr<int32_t>(),
                         (int)cap, xowner->data_ptr<int32_t>(),
                         qowner->data_ptr<int32_t>(), hist.data_ptr<int32_t>(),
                         w.data_ptr<float>(), inv_w.data_ptr<float>());
    else
      hipLaunchKernelGGL(topk_scan_fp4_hist_kernel, grid, dim3(512), 0, cur_stream(),
                         Q4.data_ptr<uint8_t>(), QS.data_ptr<uint8_t>(),
                         X4.data_ptr<uint8_t>(), XS.data_ptr<uint8_t>(),
                         nq, (int)nx, D, 1, (int)n_swaths,
                         cand_s.data_ptr<float>(), cand_i.data_ptr<int32_t>(),
                         theta.data_ptr<float>(), counts.data_ptr<int32_t>(),
                         (int)cap, hist.data_ptr<int32_t>(),
                         w.data_ptr<float>(), inv_w.data_ptr<float>());
    return {cand_s, cand_i, counts, hist};
  }
  if (xowner != nullptr) {
    hipLaunchKernelGGL(topk_scan_fp4_owned_kernel, grid, dim3(512), 0, cur_stream(),
                       Q4.data_ptr<uint8_t>(), QS.data_ptr<uint8_t>(),
                       X4.data_ptr<uint8_t>(), XS.data_ptr<uint8_t>(),
                       nq, (int)nx, D, 1, (int)n_swaths,
                       cand_s.data_ptr<float>(), cand_i.data_ptr<int32_t>(),
                       theta.data_ptr<float>(), counts.data_ptr<int32_t>(),
                       (int)cap, xowner->data_ptr<int32_t>(),
                       qowner->data_ptr<int32_t>());
    return {cand_s, cand_i, counts};
  }
  auto kern = variant == 10 ? topk_scan_fp4_v10_kernel
            : variant == 9 ? topk_scan_fp4_v9_kernel
            : variant == 7 ? topk_scan_fp4_v7_kernel
            : variant == 4 ? topk_scan_fp4_v5_kernel
            : variant == 2 ? topk_scan_fp4_v3_kernel
            : variant == 1 ? topk_scan_fp4_v2_kernel : topk_scan_fp4_kernel;
  hipLaunchKernelGGL(kern, grid, dim3(512), 0, cur_stream(),
                     Q4.data_ptr<uint8_t>(), QS.data_ptr<uint8_t>(),
                     X4.data_ptr<uint8_t>(), XS.data_ptr<uint8_t>(),
                     nq, (int)nx, D, scan_only ? -1 : 1, (int)n_swaths,
                     cand_s.data_ptr<float>(), cand_i.data_ptr<int32_t>(),
                     theta.data_ptr<float>(), counts.data_ptr<int32_t>(),
                     (int)cap);
  return {cand_s, cand_i, counts};
}

std::vector<torch::Tensor> topk_scan_threshold_fp4x4(
    torch::Tensor Q4, torch::Tensor QS, torch::Tensor X4, torch::Tensor XS,
    torch::Tensor theta, int64_t cap, int64_t n_swaths, int64_t variant_arg,
    bool scan_only) {
  return fp4x4_scan(Q4, QS, X4, XS, theta, cap, n_swaths, variant_arg, scan_only,
                    nullptr, nullptr);
}

// Owner-filtered fp4x4 threshold scan (csrc topk_scan_fp4_owned_kernel):
// appends only (query, row) pairs with qowner[query] < 0 or xowner[row] ==
// qowner[query].
std::vector<torch::Tensor> topk_scan_threshold_fp4x4_owned(
    torch::Tensor Q4, torch::Tensor QS, torch::Tensor X4, torch::Tensor XS,
    torch::Tensor theta, torch::Tensor xowner, torch::Tensor qowner, int64_t cap,
    int64_t n_swaths) {
  return fp4x4_scan(Q4, QS, X4, XS, theta, cap, n_swaths, -1, false, &xowner,
                    &qowner);
}

// fp4x4 threshold scan (v10, or the owned scan with owners) that returns a
// fourth tensor hist[nq, 256] int32, zeroed here: per query, the hits that
// found the candidate buffer full, counted in bins of width w[q] above
// theta[q] (ops.gpu.hist_bin_spec is the bin rule).
std::vector<torch::Tensor> topk_scan_threshold_fp4x4_hist(
    torch::Tensor Q4, torch::Tensor QS, torch::Tensor X4, torch::Tensor XS,
    torch::Tensor theta, torch::Tensor w, int64_t cap, int64_t n_swaths,
    c10::optional<torch::Tensor> xowner, c10::optional<torch::Tensor> qowner) {
  TORCH_CHECK(xowner.has_value() == qowner.has_value(),
              "xowner and qowner must be given together");
  bool owned = xowner.has_value();
  return fp4x4_scan(Q4, QS, X4, XS, theta, cap, n_swaths, -1, false,
                    owned ? &*xowner : nullptr, owned ? &*qowner : nullptr, &w);
}

std::vector<torch::Tensor> topk_scan_threshold(torch::Tensor Q, torch::Tensor X,
                                               torch::Tensor theta, int64_t cap,
                                               int64_t n_swaths, bool fp8, bool mx,
                                               c10::optional<torch::Tensor> xowner,
                                               c10::optional<torch::Tensor> qowner) {
  // threshold-scan mode: append every score > theta[q] to a per-query
  // candidate buffer (no top-k maintenance in-kernel)
  CHECK_GPU(Q); CHECK_CONTIG(Q); CHECK_GPU(X); CHECK_CONTIG(X);
  CHECK_GPU(theta); CHECK_CONTIG(theta);
  TORCH_CHECK(theta.dtype() == torch::kFloat32);
  int nq = Q.size(0), D = Q.size(1);
  long long nx = X.size(0);
  TORCH_CHECK(theta.numel() == nq);
  TORCH_CHECK(X.size(1) == D && D % 64 == 0);
  TORCH_CHECK(cap >= 32 && cap <= 4096);
  bool owned = have_owners(xowner, qowner, nx, nq);
  TORCH_CHECK(!owned || !(fp8 || mx),
              "owner filter: bf16 and fp4x4 scans only");
  static const int variant = [] {
    const char* e = getenv("VAINPLEX_FP4_V2");
    return (e != nullptr && e[0] == '1') ? 1 : 0;  // pipelined v2 opt-in
  }();
  int n_qblocks = (nq + 255) / 256;
  if (n_swaths <= 0) {
    int want = 256 / (n_qblocks > 0 ? n_qblocks : 1);
    n_swaths = want >= 8 ? (want / 8) * 8 : 8;
    long long max_s = nx / 256; if (max_s < 1) max_s = 1;
    if (n_swaths > max_s) n_swaths = max_s;
  }
  auto f32opts = torch::dtype(torch::kFloat32).device(Q.device());
  auto i32opts = torch::dtype(torch::kInt32).device(Q.device());
  auto cand_s = torch::full({(long long)nq, cap}, -1e30, f32opts);
  auto cand_i = torch::full({(long long)nq, cap}, -1, i32opts);
  auto counts = torch::zeros({(long long)nq}, i32opts);
  dim3 grid((unsigned)(n_qblocks * n_swaths));
  if (mx) {
    // MX-scaled x128 scan: same e4m3 bytes, unit block scales
    TORCH_CHECK(Q.dtype() == torch::kUInt8 && X.dtype() == torch::kUInt8);
    TORCH_CHECK(D % 128 == 0, "MX scan needs D % 128 == 0");
    hipLaunchKernelGGL(topk_scan_mx_kernel, grid, dim3(512), 0, cur_stream(),
                       Q.data_ptr<uint8_t>(), X.data_ptr<uint8_t>(), nq, (int)nx,
                       D, 1, (int)n_swaths, cand_s.data_ptr<float>(),
                       cand_i.data_ptr<int32_t>(), theta.data_ptr<float>(),
                       counts.data_ptr<int32_t>(), (int)cap);
  } else if (fp8) {
    TORCH_CHECK(Q.dtype() == torch::kUInt8 && X.dtype() == torch::kUInt8);
    hipLaunchKernelGGL(topk_recall_fp8_kernel, grid, dim3(512), 0, cur_stream(),
                       Q.data_ptr<uint8_t>(), X.data_ptr<uint8_t>(), nq, (int)nx,
                       D, 1, (int)n_swaths, cand_s.data_ptr<float>(),
                       cand_i.data_ptr<int32_t>(), theta.data_ptr<float>(),
                       counts.data_ptr<int32_t>(), (int)cap);
  } else {
    TORCH_CHECK(Q.dtype() == torch::kBFloat16 && X.dtype() == torch::kBFloat16);
    hipLaunchKernelGGL(topk_recall_kernel, grid, dim3(512), 0, cur_stream(),
                       reinterpret_cast<const __bf16*>(Q.data_ptr()),
                       reinterpret_cast<const __bf16*>(X.data_ptr()), nq, (int)nx,
                       D, 1, (int)n_swaths, cand_s.data_ptr<float>(),
                       cand_i.data_ptr<int32_t>(), theta.data_ptr<float>(),
                       counts.data_ptr<int32_t>(), (int)cap,
                       owned ? xowner->data_ptr<int32_t>() : nullptr,
                       owned ? qowner->data_ptr<int32_t>() : nullptr);
  }
  return {cand_s, cand_i, counts};
}

// -- fused MXFP4 quantize / index append (csrc/fp4_quantize.hip) ----------

static bool aligned16(const torch::Tensor& t) {
  return (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0;
}

static void launch_fp4_quantize_append(
    const torch::Tensor& feats, const int32_t* src_idx, long long n, long long dst_row0,
    uint16_t* index_dst, uint8_t* x4, uint8_t* xs, int32_t* owner_dst,
    const int32_t* owner_src, float* salience_dst, float salience_init,
    long long* id_dst = nullptr, long long id_base = 0) {
  if (n == 0) return;
  int D = feats.size(1);
  long long items = n * (D / 16);
  long long blocks = (items + 255) / 256;
  // memory-bound: cap the grid and stride the rest
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(fp4_quantize_append_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     cur_stream(),
                     reinterpret_cast<const uint16_t*>(feats.data_ptr()), src_idx,
                     (int)feats.size(0), n, D, dst_row0, index_dst, x4, xs, owner_dst,
                     owner_src, salience_dst, salience_init, id_dst, id_base);
}

static void check_fp4_dst(const torch::Tensor& X4, const torch::Tensor& XS, long long rows,
                          int D) {
  CHECK_GPU(X4); CHECK_CONTIG(X4); CHECK_GPU(XS); CHECK_CONTIG(XS);
  TORCH_CHECK(X4.dtype() == torch::kUInt8 && XS.dtype() == torch::kUInt8,
              "X4/XS must be uint8");
  TORCH_CHECK(X4.dim() == 2 && XS.dim() == 2 && X4.size(0) == rows && XS.size(0) == rows &&
              X4.size(1) == D / 2 && XS.size(1) == D / 32,
              "X4/XS must be [rows, D/2] and [rows, D/32]");
  TORCH_CHECK(aligned16(X4) && aligned16(XS), "X4/XS must be 16-byte aligned");
}

std::vector<torch::Tensor> quantize_fp4_mx(torch::Tensor X,
                                           c10::optional<torch::Tensor> out4,
                                           c10::optional<torch::Tensor> outs) {
  // bf16 [n, D] -> (packed e2m1 [n, D/2], e8m0 scales [n, D/32]), bit-exact
  // with ops.gpu.to_fp4_mx; out4/outs let a caller fill preallocated rows
  CHECK_GPU(X); CHECK_CONTIG(X);
  TORCH_CHECK(X.dtype() == torch::kBFloat16 && X.dim() == 2, "X must be bf16 [n, D]");
  long long n = X.size(0);
  int D = X.size(1);
  TORCH_CHECK(D % 128 == 0 && D <= 2048, "fp4 quantize needs D%128==0, D<=2048");
  TORCH_CHECK(n < (1LL << 31), "X has too many rows");
  TORCH_CHECK(aligned16(X), "X must be 16-byte aligned");
  TORCH_CHECK(out4.has_value() == outs.has_value(), "out4 and outs go together");
  auto u8opts = torch::dtype(torch::kUInt8).device(X.device());
  auto X4 = out4.has_value() ? *out4 : torch::empty({n, D / 2}, u8opts);
  auto XS = outs.has_value() ? *outs : torch::empty({n, D / 32}, u8opts);
  check_fp4_dst(X4, XS, n, D);
  launch_fp4_quantize_append(X, nullptr, n, 0, nullptr, X4.data_ptr<uint8_t>(),
                             XS.data_ptr<uint8_t>(), nullptr, nullptr, nullptr, 0.f);
  return {X4, XS};
}

void index_append(torch::Tensor feats, c10::optional<torch::Tensor> src_idx,
                  int64_t dst_row0, torch::Tensor index,
                  c10::optional<torch::Tensor> X4, c10::optional<torch::Tensor> XS,
                  c10::optional<torch::Tensor> owner_dst,
                  c10::optional<torch::Tensor> owner_src,
                  c10::optional<torch::Tensor> salience_dst, double salience_init,
                  c10::optional<torch::Tensor> id_dst, int64_t id_base) {
  // rows dst_row0 + i of the live index <- feats[src_idx[i]] (or feats[i]):
  // bf16 copy, fp4 codes + scales, owner, salience and memory id
  // (id_base + the source row) in one launch
  CHECK_GPU(feats); CHECK_CONTIG(feats); CHECK_GPU(index); CHECK_CONTIG(index);
  TORCH_CHECK(feats.dtype() == torch::kBFloat16 && feats.dim() == 2,
              "feats must be bf16 [m, D]");
  TORCH_CHECK(index.dtype() == torch::kBFloat16 && index.dim() == 2,
              "index must be bf16 [cap, D]");
  long long m = feats.size(0), cap = index.size(0);
  int D = feats.size(1);
  TORCH_CHECK(index.size(1) == D, "feats and index differ in D");
  TORCH_CHECK(D % 128 == 0 && D <= 2048, "index append needs D%128==0, D<=2048");
  TORCH_CHECK(m < (1LL << 31), "feats has too many rows");
  TORCH_CHECK(aligned16(feats) && aligned16(index), "feats/index must be 16-byte aligned");
  TORCH_CHECK(feats.device() == index.device(), "feats and index on different devices");
  long long n = m;
  const int32_t* sp = nullptr;
  if (src_idx.has_value()) {
    CHECK_GPU((*src_idx)); CHECK_CONTIG((*src_idx));
    TORCH_CHECK(src_idx->dtype() == torch::kInt32 && src_idx->dim() == 1,
                "src_idx must be int32 [n]");
    n = src_idx->numel();
    sp = src_idx->data_ptr<int32_t>();
  }
  TORCH_CHECK(dst_row0 >= 0 && dst_row0 + n <= cap,
              "index append window [", dst_row0, ", ", dst_row0 + n, ") exceeds capacity ", cap);
  TORCH_CHECK(X4.has_value() == XS.has_value(), "X4 and XS go together");
  uint8_t* x4p = nullptr; uint8_t* xsp = nullptr;
  if (X4.has_value()) {
    check_fp4_dst(*X4, *XS, cap, D);
    x4p = X4->data_ptr<uint8_t>();
    xsp = XS->data_ptr<uint8_t>();
  }
  TORCH_CHECK(owner_dst.has_value() == owner_src.has_value(),
              "owner_dst and owner_src go together");
  int32_t* odp = nullptr; const int32_t* osp = nullptr;
  if (owner_dst.has_value()) {
    CHECK_GPU((*owner_dst)); CHECK_CONTIG((*owner_dst));
    CHECK_GPU((*owner_src)); CHECK_CONTIG((*owner_src));
    TORCH_CHECK(owner_dst->dtype() == torch::kInt32 && owner_src->dtype() == torch::kInt32,
                "owners must be int32");
    TORCH_CHECK(owner_dst->dim() == 1 && owner_dst->numel() == cap, "owner_dst must be [cap]");
    TORCH_CHECK(owner_src->dim() == 1 && owner_src->numel() == m, "owner_src must be [m]");
    odp = owner_dst->data_ptr<int32_t>();
    osp = owner_src->data_ptr<int32_t>();
  }
  float* sdp = nullptr;
  if (salience_dst.has_value()) {
    CHECK_GPU((*salience_dst)); CHECK_CONTIG((*salience_dst));
    TORCH_CHECK(salience_dst->dtype() == torch::kFloat32 && salience_dst->dim() == 1 &&
                salience_dst->numel() == cap, "salience_dst must be f32 [cap]");
    sdp = salience_dst->data_ptr<float>();
  }
  long long* idp = nullptr;
  if (id_dst.has_value()) {
    CHECK_GPU((*id_dst)); CHECK_CONTIG((*id_dst));
    TORCH_CHECK(id_dst->dtype() == torch::kInt64 && id_dst->dim() == 1 &&
                id_dst->numel() == cap, "id_dst must be int64 [cap]");
    TORCH_CHECK(id_dst->device() == index.device(), "id_dst and index on different devices");
    idp = reinterpret_cast<long long*>(id_dst->data_ptr<int64_t>());
  }
  launch_fp4_quantize_append(feats, sp, n, dst_row0,
                             reinterpret_cast<uint16_t*>(index.data_ptr()), x4p, xsp, odp,
                             osp, sdp, (float)salience_init, idp, (long long)id_base);
}

// -- forgetting: in-place row moves (csrc/index_forget.hip) ----------------

void index_move_rows(torch::Tensor src, torch::Tensor dst,
                     c10::optional<torch::Tensor> index,
                     c10::optional<torch::Tensor> X4, c10::optional<torch::Tensor> XS,
                     c10::optional<torch::Tensor> owner,
                     c10::optional<torch::Tensor> salience,
                     c10::optional<torch::Tensor> ids) {
  // row dst[j] of every given buffer <- row src[j], bitwise, in one launch;
  // a pair with an index outside [0, cap) is skipped by the kernel
  CHECK_GPU(src); CHECK_CONTIG(src); CHECK_GPU(dst); CHECK_CONTIG(dst);
  TORCH_CHECK(src.dtype() == torch::kInt32 && dst.dtype() == torch::kInt32 &&
              src.dim() == 1 && dst.dim() == 1, "src/dst must be int32 [m]");
  TORCH_CHECK(src.numel() == dst.numel(), "src and dst differ in length");
  TORCH_CHECK(src.device() == dst.device(), "src and dst on different devices");
  TORCH_CHECK(index.has_value() || X4.has_value() || owner.has_value() ||
              salience.has_value() || ids.has_value(),
              "index_move_rows needs at least one buffer");
  TORCH_CHECK(X4.has_value() == XS.has_value(), "X4 and XS go together");
  long long cap = -1;
  int D = 0;
  auto same_cap = [&](const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.device() == src.device(), name, " and src on different devices");
    if (cap < 0) cap = t.size(0);
    TORCH_CHECK(t.size(0) == cap, name, " differs in capacity from the other buffers");
  };
  uint4* ip = nullptr;
  if (index.has_value()) {
    CHECK_GPU((*index)); CHECK_CONTIG((*index));
    TORCH_CHECK(index->dtype() == torch::kBFloat16 && index->dim() == 2,
                "index must be bf16 [cap, D]");
    D = index->size(1);
    TORCH_CHECK(D > 0 && D % 8 == 0, "index rows must be a multiple of 16 bytes (D%8==0)");
    TORCH_CHECK(aligned16(*index), "index must be 16-byte aligned");
    same_cap(*index, "index");
    ip = reinterpret_cast<uint4*>(index->data_ptr());
  }
  uint4* x4p = nullptr; uint32_t* xsp = nullptr;
  if (X4.has_value()) {
    TORCH_CHECK(X4->dim() == 2, "X4 must be [cap, D/2]");
    int D4 = (int)X4->size(1) * 2;
    TORCH_CHECK(!index.has_value() || D4 == D, "index and X4 differ in D");
    D = D4;
    TORCH_CHECK(D > 0 && D % 128 == 0 && D <= 2048, "fp4 rows need D%128==0, D<=2048");
    check_fp4_dst(*X4, *XS, X4->size(0), D);
    same_cap(*X4, "X4");
    same_cap(*XS, "XS");
    x4p = reinterpret_cast<uint4*>(X4->data_ptr());
    xsp = reinterpret_cast<uint32_t*>(XS->data_ptr());
  }
  uint32_t* op = nullptr;
  if (owner.has_value()) {
    CHECK_GPU((*owner)); CHECK_CONTIG((*owner));
    TORCH_CHECK(owner->dtype() == torch::kInt32 && owner->dim() == 1, "owner must be int32 [cap]");
    same_cap(*owner, "owner");
    op = reinterpret_cast<uint32_t*>(owner->data_ptr());
  }
  uint32_t* sp = nullptr;
  if (salience.has_value()) {
    CHECK_GPU((*salience)); CHECK_CONTIG((*salience));
    TORCH_CHECK(salience->dtype() == torch::kFloat32 && salience->dim() == 1,
                "salience must be f32 [cap]");
    same_cap(*salience, "salience");
    sp = reinterpret_cast<uint32_t*>(salience->data_ptr());
  }
  uint2* idp = nullptr;
  if (ids.has_value()) {
    CHECK_GPU((*ids)); CHECK_CONTIG((*ids));
    TORCH_CHECK(ids->dtype() == torch::kInt64 && ids->dim() == 1, "ids must be int64 [cap]");
    same_cap(*ids, "ids");
    idp = reinterpret_cast<uint2*>(ids->data_ptr());
  }
  TORCH_CHECK(cap < (1LL << 31), "index has too many rows");
  long long m = src.numel();
  if (m == 0) return;
  // one wave per pair, 4 waves per block; memory-bound: cap the grid and
  // stride the rest
  long long blocks = (m + 3) / 4;
  if (blocks > 256 * 8) blocks = 256 * 8;
  hipLaunchKernelGGL(index_move_rows_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     cur_stream(), src.data_ptr<int32_t>(), dst.data_ptr<int32_t>(), m,
                     (int)cap, D, ip, x4p, xsp, op, sp, idp);
}

// -- memory ids: rows by id (csrc/index_ids.hip) ----------------------------

void index_find_ids(torch::Tensor col, torch::Tensor want, torch::Tensor row_out) {
  // row_out[j] <- max(row_out[j], highest row of col holding want[j]); want
  // is one chunk, ascending and distinct; the caller prefills row_out with -1
  CHECK_GPU(col); CHECK_CONTIG(col); CHECK_GPU(want); CHECK_CONTIG(want);
  CHECK_GPU(row_out); CHECK_CONTIG(row_out);
  TORCH_CHECK(col.dtype() == torch::kInt64 && col.dim() == 1, "col must be int64 [n]");
  TORCH_CHECK(want.dtype() == torch::kInt64 && want.dim() == 1, "want must be int64 [m]");
  TORCH_CHECK(row_out.dtype() == torch::kInt32 && row_out.dim() == 1 &&
              row_out.numel() == want.numel(), "row_out must be int32 [m]");
  TORCH_CHECK(col.device() == want.device() && col.device() == row_out.device(),
              "col, want and row_out on different devices");
  long long n = col.numel(), m = want.numel();
  TORCH_CHECK(n < (1LL << 31), "col has too many rows");
  TORCH_CHECK(m <= 4096, "want holds more than one chunk (4096 ids)");
  if (n == 0 || m == 0) return;
  // one 16-byte pair per lane; 32 KB of LDS a block, so 4 blocks a CU at most
  long long blocks = (n / 2 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 256 * 4) blocks = 256 * 4;
  hipLaunchKernelGGL(index_find_ids_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     cur_stream(), reinterpret_cast<const long long*>(col.data_ptr<int64_t>()),
                     n, reinterpret_cast<const long long*>(want.data_ptr<int64_t>()), (int)m,
                     row_out.data_ptr<int32_t>());
}

// -- ingest dedup: near-duplicate detection (csrc/ingest_dedup.hip) --------

void batch_first_similar(torch::Tensor F, torch::Tensor elig, double tau,
                         c10::optional<torch::Tensor> owner, torch::Tensor first) {
  // first[i] <- min(first[i], smallest eligible same-owner j < i with
  // dot(F_i, F_j) >= tau); the caller presets first (i if eligible, else -1)
  CHECK_GPU(F); CHECK_CONTIG(F); CHECK_GPU(elig); CHECK_CONTIG(elig);
  CHECK_GPU(first); CHECK_CONTIG(first);
  TORCH_CHECK(F.dtype() == torch::kBFloat16 && F.dim() == 2, "F must be bf16 [B, D]");
  long long B = F.size(0);
  int D = F.size(1);
  TORCH_CHECK(B >= 1 && B <= (1LL << 22), "batch_first_similar needs 1 <= B <= 2^22");
  TORCH_CHECK(D > 0 && D % 32 == 0, "batch_first_similar needs D % 32 == 0");
  TORCH_CHECK(aligned16(F), "F must be 16-byte aligned");
  TORCH_CHECK((elig.dtype() == torch::kBool || elig.dtype() == torch::kUInt8) &&
              elig.dim() == 1 && elig.numel() == B, "elig must be bool [B]");
  TORCH_CHECK(first.dtype() == torch::kInt32 && first.dim() == 1 && first.numel() == B,
              "first must be int32 [B]");
  TORCH_CHECK(elig.device() == F.device() && first.device() == F.device(),
              "F, elig and first on different devices");
  const int32_t* op = nullptr;
  if (owner.has_value()) {
    CHECK_GPU((*owner)); CHECK_CONTIG((*owner));
    TORCH_CHECK(owner->dtype() == torch::kInt32 && owner->dim() == 1 && owner->numel() == B,
                "owner must be int32 [B]");
    TORCH_CHECK(owner->device() == F.device(), "F and owner on different devices");
    op = owner->data_ptr<int32_t>();
  }
  unsigned tiles = (unsigned)((B + 127) / 128);
  hipLaunchKernelGGL(batch_first_similar_kernel, dim3(tiles, tiles), dim3(256), 0,
                     cur_stream(), reinterpret_cast<const __bf16*>(F.data_ptr()),
                     reinterpret_cast<const uint8_t*>(elig.data_ptr()), op, (int)B, D,
                     (float)tau, first.data_ptr<int32_t>());
}

std::vector<torch::Tensor> recall_dup_rows(torch::Tensor F, torch::Tensor ids,
                                           torch::Tensor X, double tau,
                                           c10::optional<torch::Tensor> xowner,
                                           c10::optional<torch::Tensor> qowner) {
  // per message the recalled row with the largest dot >= tau (ties: lowest
  // id), -1 if none; ids are bounds-checked by the kernel
  CHECK_GPU(F); CHECK_CONTIG(F); CHECK_GPU(ids); CHECK_CONTIG(ids);
  CHECK_GPU(X); CHECK_CONTIG(X);
  TORCH_CHECK(F.dtype() == torch::kBFloat16 && F.dim() == 2, "F must be bf16 [B, D]");
  TORCH_CHECK(X.dtype() == torch::kBFloat16 && X.dim() == 2, "X must be bf16 [n, D]");
  long long B = F.size(0), n = X.size(0);
  int D = F.size(1);
  TORCH_CHECK(X.size(1) == D, "F and X differ in D");
  TORCH_CHECK(D > 0 && D % 8 == 0 && D <= 2048, "recall_dup_rows needs D%8==0, D<=2048");
  TORCH_CHECK(B < (1LL << 31) && n < (1LL << 31), "too many rows");
  TORCH_CHECK(aligned16(F) && aligned16(X), "F and X must be 16-byte aligned");
  TORCH_CHECK(ids.dtype() == torch::kInt32 && ids.dim() == 2 && ids.size(0) == B,
              "ids must be int32 [B, k]");
  TORCH_CHECK(ids.device() == F.device() && X.device() == F.device(),
              "F, ids and X on different devices");
  int k = ids.size(1);
  TORCH_CHECK(xowner.has_value() == qowner.has_value(), "xowner and qowner go together");
  const int32_t* xop = nullptr; const int32_t* qop = nullptr;
  if (xowner.has_value()) {
    CHECK_GPU((*xowner)); CHECK_CONTIG((*xowner));
    CHECK_GPU((*qowner)); CHECK_CONTIG((*qowner));
    TORCH_CHECK(xowner->dtype() == torch::kInt32 && qowner->dtype() == torch::kInt32,
                "owners must be int32");
    TORCH_CHECK(xowner->dim() == 1 && xowner->numel() == n, "xowner must be [n]");
    TORCH_CHECK(qowner->dim() == 1 && qowner->numel() == B, "qowner must be [B]");
    TORCH_CHECK(xowner->device() == F.device() && qowner->device() == F.device(),
                "owners on another device than F");
    xop = xowner->data_ptr<int32_t>();
    qop = qowner->data_ptr<int32_t>();
  }
  auto dup_row = torch::empty({B}, torch::dtype(torch::kInt32).device(F.device()));
  auto dup_dot = torch::empty({B}, torch::dtype(torch::kFloat32).device(F.device()));
  if (B == 0) return {dup_row, dup_dot};
  // one wave per message, 4 waves per block; cap the grid, stride the rest
  long long blocks = (B + 3) / 4;
  if (blocks > 256 * 8) blocks = 256 * 8;
  hipLaunchKernelGGL(recall_dup_rows_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     cur_stream(), reinterpret_cast<const uint4*>(F.data_ptr()),
                     ids.data_ptr<int32_t>(), reinterpret_cast<const uint4*>(X.data_ptr()),
                     xop, qop, (int)B, k, D, (int)n, (float)tau,
                     dup_row.data_ptr<int32_t>(), dup_dot.data_ptr<float>());
  return {dup_row, dup_dot};
}

// csrc/recall_epilogue.hip: mean and correction=1 std of every row of a bf16
// matrix, one pass, fp64 sums in a fixed order. Returns (mu, sigma) fp32 [nq].
std::vector<torch::Tensor> row_moments(torch::Tensor S) {
  CHECK_GPU(S); CHECK_CONTIG(S);
  TORCH_CHECK(S.dtype() == torch::kBFloat16 && S.dim() == 2, "S must be bf16 [nq, m]");
  long long nq = S.size(0), m = S.size(1);
  TORCH_CHECK(m >= 1 && m < (1LL << 31) && nq < (1LL << 31), "row_moments: bad shape");
  auto mu = torch::empty({nq}, torch::dtype(torch::kFloat32).device(S.device()));
  auto sigma = torch::empty({nq}, torch::dtype(torch::kFloat32).device(S.device()));
  if (nq == 0) return {mu, sigma};
  hipLaunchKernelGGL(row_moments_kernel, dim3((unsigned)nq), dim3(256), 0, cur_stream(),
                     reinterpret_cast<const uint16_t*>(S.data_ptr()), (int)m,
                     mu.data_ptr<float>(), sigma.data_ptr<float>());
  return {mu, sigma};
}

// csrc/recall_epilogue.hip: candidate select by scan score, exact fp32
// rescore, salience weight and top-k, one block per query. The shapes it
// takes are the ones ops.gpu.select_rescore routes here.
std::vector<torch::Tensor> select_rescore(torch::Tensor cs, torch::Tensor ci,
                                          torch::Tensor counts, torch::Tensor Q,
                                          torch::Tensor X,
                                          c10::optional<torch::Tensor> salience,
                                          int64_t sel, int64_t k) {
  CHECK_GPU(cs); CHECK_CONTIG(cs); CHECK_GPU(ci); CHECK_CONTIG(ci);
  CHECK_GPU(counts); CHECK_CONTIG(counts);
  CHECK_GPU(Q); CHECK_CONTIG(Q); CHECK_GPU(X); CHECK_CONTIG(X);
  TORCH_CHECK(Q.dtype() == torch::kBFloat16 && Q.dim() == 2, "Q must be bf16 [nq, D]");
  TORCH_CHECK(X.dtype() == torch::kBFloat16 && X.dim() == 2, "X must be bf16 [nx, D]");
  long long nq = Q.size(0), nx = X.size(0);
  int D = Q.size(1);
  TORCH_CHECK(X.size(1) == D, "Q and X differ in D");
  TORCH_CHECK(D > 0 && D % 8 == 0 && D <= 2048, "select_rescore needs D%8==0, D<=2048");
  TORCH_CHECK(nq < (1LL << 31) && nx < (1LL << 31), "too many rows");
  TORCH_CHECK(aligned16(Q) && aligned16(X), "Q and X must be 16-byte aligned");
  TORCH_CHECK(cs.dtype() == torch::kFloat32 && cs.dim() == 2 && cs.size(0) == nq,
              "cs must be fp32 [nq, cap]");
  long long cap = cs.size(1);
  TORCH_CHECK(ci.dtype() == torch::kInt32 && ci.dim() == 2 && ci.size(0) == nq &&
              ci.size(1) == cap, "ci must be int32 [nq, cap]");
  TORCH_CHECK(counts.dtype() == torch::kInt32 && counts.dim() == 1 && counts.numel() == nq,
              "counts must be int32 [nq]");
  TORCH_CHECK(cap >= 1 && cap <= 1024 && k >= 1 && k <= sel && sel <= cap,
              "select_rescore needs 1 <= k <= sel <= cap <= 1024");
  TORCH_CHECK(cs.device() == Q.device() && ci.device() == Q.device() &&
              counts.device() == Q.device() && X.device() == Q.device(),
              "select_rescore: tensors on different devices");
  const float* sal = nullptr;
  if (salience.has_value()) {
    CHECK_GPU((*salience)); CHECK_CONTIG((*salience));
    TORCH_CHECK(salience->dtype() == torch::kFloat32 && salience->dim() == 1 &&
                salience->numel() >= nx && salience->device() == Q.device(),
                "salience must be fp32 [>= nx] on Q's device");
    sal = salience->data_ptr<float>();
  }
  auto out_s = torch::empty({nq, k}, torch::dtype(torch::kFloat32).device(Q.device()));
  auto out_i = torch::empty({nq, k}, torch::dtype(torch::kInt32).device(Q.device()));
  if (nq == 0) return {out_s, out_i};
  hipLaunchKernelGGL(select_rescore_kernel, dim3((unsigned)nq), dim3(256), 0, cur_stream(),
                     cs.data_ptr<float>(), ci.data_ptr<int32_t>(), counts.data_ptr<int32_t>(),
                     reinterpret_cast<const uint4*>(Q.data_ptr()),
                     reinterpret_cast<const uint4*>(X.data_ptr()), sal, (int)cap, (int)sel,
                     (int)k, D, (int)nx, out_s.data_ptr<float>(), out_i.data_ptr<int32_t>());
  return {out_s, out_i};
}

void register_host_envelope(pybind11::module_& m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  register_host_envelope(m);
  m.def("sha256_leaves", &sha256_leaves, "Batched SHA-256 leaf digests");
  m.def("merkle_root", &merkle_root_gpu, "Merkle root over leaf digests");
  m.def("dfa_scan", &dfa_scan, "Multi-pattern DFA scan");
  m.def("dfa_scan_multi", &dfa_scan_multi, "All-family DFA scan in one launch");
  m.def("fact_probe", &fact_probe, "GPU fact-registry hash probe");
  m.def("encode_messages", &encode_messages, "4-gram hash embedding encoder");
  m.def("gemm_nt", &gemm_nt, "bf16 NT GEMM with fused epilogue",
        py::arg("A"), py::arg("B"), py::arg("bias") = c10::nullopt,
        py::arg("act") = 0, py::arg("out_bf16") = false);
  m.def("topk_recall", &topk_recall, "Fused cosine top-k recall",
        py::arg("Q"), py::arg("X"), py::arg("k"), py::arg("n_swaths"),
        py::arg("xowner") = c10::nullopt, py::arg("qowner") = c10::nullopt);
  m.def("topk_scan_only", [](torch::Tensor Q, torch::Tensor X, int64_t n_swaths, bool fp8,
                             bool mx) {
    // perf diagnosis: run the scan loop with the top-k phase skipped
    CHECK_GPU(Q); CHECK_GPU(X);
    int nq = Q.size(0), D = Q.size(1);
    long long nx = X.size(0);
    int n_qblocks = (nq + 255) / 256;
    auto f32opts = torch::dtype(torch::kFloat32).device(Q.device());
    auto i32opts = torch::dtype(torch::kInt32).device(Q.device());
    auto cand_s = torch::zeros({(long long)n_qblocks * n_swaths * 256}, f32opts);
    auto cand_i = torch::zeros({1}, i32opts);
    dim3 grid((unsigned)(n_qblocks * n_swaths));
    if (mx) {
      hipLaunchKernelGGL(topk_scan_mx_kernel, grid, dim3(512), 0, cur_stream(),
                         Q.data_ptr<uint8_t>(), X.data_ptr<uint8_t>(), nq, (int)nx,
                         D, -1, (int)n_swaths, cand_s.data_ptr<float>(),
                         cand_i.data_ptr<int32_t>(), nullptr, nullptr, 0);
    } else if (fp8) {
      hipLaunchKernelGGL(topk_recall_fp8_kernel, grid, dim3(512), 0, cur_stream(),
                         Q.data_ptr<uint8_t>(), X.data_ptr<uint8_t>(), nq, (int)nx,
                         D, -1, (int)n_swaths, cand_s.data_ptr<float>(),
                         cand_i.data_ptr<int32_t>(), nullptr, nullptr, 0);
    } else {
      hipLaunchKernelGGL(topk_recall_kernel, grid, dim3(512), 0, cur_stream(),
                         reinterpret_cast<const __bf16*>(Q.data_ptr()),
                         reinterpret_cast<const __bf16*>(X.data_ptr()), nq, (int)nx,
                         D, -1, (int)n_swaths, cand_s.data_ptr<float>(),
                         cand_i.data_ptr<int32_t>(), nullptr, nullptr, 0,
                         nullptr, nullptr);
    }
  }, "scan-only diagnosis", py::arg("Q"), py::arg("X"), py::arg("n_swaths"),
     py::arg("fp8") = false, py::arg("mx") = false);
  m.def("topk_recall_fp8", &topk_recall_fp8, "fp8 stage-1 scan of two-stage recall");
  m.def("topk_scan_threshold", &topk_scan_threshold,
        "threshold-scan candidate collection (bf16, fp8 or MX-fp8)",
        py::arg("Q"), py::arg("X"), py::arg("theta"), py::arg("cap"),
        py::arg("n_swaths"), py::arg("fp8") = false, py::arg("mx") = false,
        py::arg("xowner") = c10::nullopt, py::arg("qowner") = c10::nullopt);
  m.def("topk_scan_threshold_fp4",
        [](torch::Tensor Q8, torch::Tensor X4, torch::Tensor XS,
           torch::Tensor theta, int64_t cap, int64_t n_swaths) {
    // MXFP4 X operand: X4 = packed e2m1 nibbles [nx, D/2], XS = e8m0
    // block scales [nx, D/32]; Q8 stays e4m3. Scores are x8 (Q scale only).
    CHECK_GPU(Q8); CHECK_CONTIG(Q8); CHECK_GPU(X4); CHECK_CONTIG(X4);
    CHECK_GPU(XS); CHECK_CONTIG(XS); CHECK_GPU(theta); CHECK_CONTIG(theta);
    TORCH_CHECK(Q8.dtype() == torch::kUInt8 && X4.dtype() == torch::kUInt8 &&
                XS.dtype() == torch::kUInt8);
    TORCH_CHECK(theta.dtype() == torch::kFloat32);
    int nq = Q8.size(0), D = Q8.size(1);
    long long nx = X4.size(0);
    TORCH_CHECK(D % 128 == 0 && D / 32 <= 64, "fp4 scan needs D%128==0, D<=2048");
    TORCH_CHECK(X4.size(1) == D / 2 && XS.size(0) == nx && XS.size(1) == D / 32);
    TORCH_CHECK(theta.numel() == nq);
    TORCH_CHECK(cap >= 32 && cap <= 4096);
    int n_qblocks = (nq + 255) / 256;
    if (n_swaths <= 0) {
      int want = 256 / (n_qblocks > 0 ? n_qblocks : 1);
      n_swaths = want >= 8 ? (want / 8) * 8 : 8;
      long long max_s = nx / 256; if (max_s < 1) max_s = 1;
      if (n_swaths > max_s) n_swaths = max_s;
    }
    auto f32opts = torch::dtype(torch::kFloat32).device(Q8.device());
    auto i32opts = torch::dtype(torch::kInt32).device(Q8.device());
    auto cand_s = torch::full({(long long)nq, cap}, -1e30, f32opts);
    auto cand_i = torch::full({(long long)nq, cap}, -1, i32opts);
    auto counts = torch::zeros({(long long)nq}, i32opts);
    dim3 grid((unsigned)(n_qblocks * n_swaths));
    hipLaunchKernelGGL(topk_scan_mx4_kernel, grid, dim3(512), 0, cur_stream(),
                       Q8.data_ptr<uint8_t>(), X4.data_ptr<uint8_t>(),
                       XS.data_ptr<uint8_t>(), nq, (int)nx, D, 1, (int)n_swaths,
                       cand_s.data_ptr<float>(), cand_i.data_ptr<int32_t>(),
                       theta.data_ptr<float>(), counts.data_ptr<int32_t>(),
                       (int)cap);
    return std::vector<torch::Tensor>{cand_s, cand_i, counts};
  }, "MXFP4-X threshold scan");
  m.def("topk_scan_threshold_fp4x4", &topk_scan_threshold_fp4x4,
        "full-MXFP4 threshold scan (both operands e2m1 + e8m0 group scales)",
        py::arg("Q4"), py::arg("QS"), py::arg("X4"), py::arg("XS"),
        py::arg("theta"), py::arg("cap"), py::arg("n_swaths"),
        py::arg("variant") = -1, py::arg("scan_only") = false);
  m.def("topk_scan_threshold_fp4x4_owned", &topk_scan_threshold_fp4x4_owned,
        "owner-filtered full-MXFP4 threshold scan (agent-isolated recall)",
        py::arg("Q4"), py::arg("QS"), py::arg("X4"), py::arg("XS"),
        py::arg("theta"), py::arg("xowner"), py::arg("qowner"), py::arg("cap"),
        py::arg("n_swaths"));
  m.def("topk_scan_threshold_fp4x4_hist", &topk_scan_threshold_fp4x4_hist,
        "full-MXFP4 threshold scan + per-query histogram of the dropped hits",
        py::arg("Q4"), py::arg("QS"), py::arg("X4"), py::arg("XS"),
        py::arg("theta"), py::arg("w"), py::arg("cap"), py::arg("n_swaths"),
        py::arg("xowner") = c10::nullopt, py::arg("qowner") = c10::nullopt);
  m.def("quantize_fp4_mx", &quantize_fp4_mx,
        "fused bf16 -> MXFP4 (fragment order) quantize, bit-exact with to_fp4_mx",
        py::arg("X"), py::arg("out4") = c10::nullopt, py::arg("outs") = c10::nullopt);
  m.def("index_append", &index_append,
        "append rows to the live recall index: bf16 + fp4 + scales + owner + salience",
        py::arg("feats"), py::arg("src_idx"), py::arg("dst_row0"), py::arg("index"),
        py::arg("X4") = c10::nullopt, py::arg("XS") = c10::nullopt,
        py::arg("owner_dst") = c10::nullopt, py::arg("owner_src") = c10::nullopt,
        py::arg("salience_dst") = c10::nullopt, py::arg("salience_init") = 1.0,
        py::arg("id_dst") = c10::nullopt, py::arg("id_base") = 0);
  m.def("index_move_rows", &index_move_rows,
        "move rows src[j] onto rows dst[j] of the live recall index buffers, in place",
        py::arg("src"), py::arg("dst"), py::arg("index") = c10::nullopt,
        py::arg("X4") = c10::nullopt, py::arg("XS") = c10::nullopt,
        py::arg("owner") = c10::nullopt, py::arg("salience") = c10::nullopt,
        py::arg("ids") = c10::nullopt);
  m.def("index_find_ids", &index_find_ids,
        "rows of an id column holding each id of one sorted, distinct chunk (atomicMax)",
        py::arg("col"), py::arg("want"), py::arg("row_out"));
  m.def("batch_first_similar", &batch_first_similar,
        "ingest dedup: lower first[i] to the earliest similar eligible row j < i",
        py::arg("F"), py::arg("elig"), py::arg("tau"), py::arg("owner"), py::arg("first"));
  m.def("recall_dup_rows", &recall_dup_rows,
        "ingest dedup: per message the recalled index row with the largest dot >= tau",
        py::arg("F"), py::arg("ids"), py::arg("X"), py::arg("tau"),
        py::arg("xowner") = c10::nullopt, py::arg("qowner") = c10::nullopt);
  m.def("row_moments", &row_moments,
        "per-row mean and correction=1 std of a bf16 matrix in one pass", py::arg("S"));
  m.def("select_rescore", &select_rescore,
        "threshold recall epilogue: select by scan score, exact rescore, salience, top-k",
        py::arg("cs"), py::arg("ci"), py::arg("counts"), py::arg("Q"), py::arg("X"),
        py::arg("salience") = c10::nullopt, py::arg("sel"), py::arg("k"));
  m.def("edit_distance", [](torch::Tensor bytes, torch::Tensor offsets) {
    // batched Levenshtein over string PAIRS: offsets has 2*n+1 entries;
    // pair i = strings (2i, 2i+1) in the packed byte buffer
    CHECK_GPU(bytes); CHECK_CONTIG(bytes); CHECK_GPU(offsets); CHECK_CONTIG(offsets);
    TORCH_CHECK(bytes.dtype() == torch::kUInt8 && offsets.dtype() == torch::kInt32);
    TORCH_CHECK(offsets.numel() % 2 == 1, "offsets must cover 2*n strings");
    int n_pairs = (int)(offsets.numel() / 2);
    auto out = torch::empty({n_pairs}, torch::dtype(torch::kInt32).device(bytes.device()));
    if (n_pairs > 0)
      hipLaunchKernelGGL(edit_distance_kernel, dim3(n_pairs), dim3(64), 0, cur_stream(),
                         bytes.data_ptr<uint8_t>(), offsets.data_ptr<int32_t>(),
                         out.data_ptr<int32_t>(), n_pairs);
    return out;
  }, "Batched Levenshtein edit distance (wavefront DP)");
  m.def("firewall_verdict", &firewall_verdict, "Fused verdict/risk/trust-delta");
  m.def("trust_recompute", &trust_recompute, "Agent trust score recompute");
  m.def("audit_pack", &audit_pack, "Pack 64-byte audit records");
}
