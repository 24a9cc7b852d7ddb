// Sanitizer driver (test infrastructure): the SuperGlue family's host-only code -- the weight
// packer (BatchNorm and merge folds, head-major permutation), every size query over tiny,
// ragged and large shapes, and the argument checks that refuse a call before anything is
// launched -- in a host-only -fsanitize=address,undefined build of onepose_amd/csrc (no GPU call
// is made).  Built and run by tests/test_superglue_sanitize.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "onepose_hip.h"

namespace {
unsigned s = 2025u;
float frand() {
  s = s * 1664525u + 1013904223u;
  return (float)((s >> 8) / 16777216.0 - 0.5);
}
}  // namespace

int main() {
  if (onepose_abi_version() != 9 || onepose_superglue_version() != 1) return 1;
  // packer: exactly-sized tensors, so a read past any of them is reported
  {
    const int n = onepose_superglue_num_tensors();
    if (n != 1 + 26 + 18 * 16 + 2) return 2;
    if (onepose_superglue_tensor_name(-1) || onepose_superglue_tensor_name(n)) return 3;
    if (onepose_superglue_tensor_numel(n) != -1) return 3;
    std::vector<std::vector<float>> t(n);
    std::vector<const float*> p(n);
    for (int i = 0; i < n; ++i) {
      const char* name = onepose_superglue_tensor_name(i);
      if (!name) return 4;
      t[i].resize((size_t)onepose_superglue_tensor_numel(i));
      const bool var = std::strstr(name, "running_var") != nullptr;
      for (float& x : t[i]) x = var ? 1.0f + frand() : frand();
      p[i] = t[i].data();
    }
    std::vector<unsigned char> packed(onepose_superglue_packed_bytes());
    if (onepose_superglue_pack(p.data(), n, packed.data()) != ONEPOSE_OK) return 5;
    if (onepose_superglue_pack(p.data(), n - 1, packed.data()) == ONEPOSE_OK) return 6;
    const float* keep = p[3];
    p[3] = nullptr;
    if (onepose_superglue_pack(p.data(), n, packed.data()) == ONEPOSE_OK) return 7;
    p[3] = keep;
    if (onepose_superglue_pack(p.data(), n, nullptr) == ONEPOSE_OK) return 8;
    std::printf("superglue pack: %d tensors, %zu bytes\n", n, packed.size());
  }
  // size queries: tiny, ragged, the chunk thresholds of the column pass, large, refused
  const int shapes[][3] = {{1, 1, 1},       {1, 1, 70},       {1, 65, 33},     {1, 300, 257},
                           {3, 130, 200},   {1, 255, 256},    {1, 256, 255},   {1, 257, 129},
                           {15, 1024, 1024}, {1, 2048, 2048}, {1, 8192, 8192}, {2, 16384, 16384},
                           {64, 4096, 4096}};
  size_t acc = 0;
  for (const auto& sh : shapes) {
    const size_t ws = onepose_superglue_workspace_bytes(sh[0], sh[1], sh[2]);
    const size_t ot = onepose_log_optimal_transport_workspace_bytes(sh[0], sh[1], sh[2]);
    // the score matrix alone is batch * n0 * n1 floats: a size that overflowed would be smaller
    if (ws < (size_t)sh[0] * sh[1] * sh[2] * 4 || ot == 0 || ot > ws) return 9;
    acc += ws + ot;
  }
  const int refused[][3] = {{0, 4, 4}, {1, 0, 4}, {1, 4, 0}, {1, -1, 4}, {1, 16385, 4},
                            {1, 4, 16385}, {65536, 4, 4}};
  for (const auto& sh : refused)
    if (onepose_superglue_workspace_bytes(sh[0], sh[1], sh[2]) != 0 ||
        onepose_log_optimal_transport_workspace_bytes(sh[0], sh[1], sh[2]) != 0)
      return 10;
  // argument checks (dummy, never dereferenced pointers: each call returns before a launch)
  {
    float* d = reinterpret_cast<float*>(uintptr_t(4096));
    int64_t* i = reinterpret_cast<int64_t*>(uintptr_t(4096));
    auto match = [&](int prec, int n0, int iters, void* ws, size_t bytes) {
      return onepose_superglue_match(d, d, 0, d, 0, d, 0, d, 0, d, 0, d, 0, 1, n0, 6, 480, 640, 480,
                                     640, iters, 0.2f, prec, i, i, d, d, nullptr, ws, bytes, nullptr);
    };
    if (match(ONEPOSE_PREC_BF16_ATTN, 5, 10, d, 1u << 30) != ONEPOSE_ERR_UNSUPPORTED) return 11;
    if (match(ONEPOSE_PREC_FP32, 0, 10, d, 1u << 30) != ONEPOSE_ERR_INVALID) return 12;
    if (match(ONEPOSE_PREC_FP32, 5, -1, d, 1u << 30) != ONEPOSE_ERR_INVALID) return 13;
    if (match(ONEPOSE_PREC_FP32, 5, 10, nullptr, 1u << 30) != ONEPOSE_ERR_INVALID) return 14;
    if (match(ONEPOSE_PREC_FP32, 5, 10, d, 8) != ONEPOSE_ERR_WORKSPACE) return 15;
    if (!*onepose_last_error()) return 16;
    if (onepose_log_optimal_transport(d, 0, 1, 4, 4, 1.f, -1, d, d, 1u << 30, nullptr) !=
        ONEPOSE_ERR_INVALID)
      return 17;
    if (onepose_log_optimal_transport(d, 0, 1, 4, 4, 1.f, 1, d, d, 8, nullptr) !=
        ONEPOSE_ERR_WORKSPACE)
      return 18;
    if (onepose_mha_softmax(d, 0, d, 0, d, 0, 1, 0, 4, d, 0, nullptr) != ONEPOSE_ERR_INVALID) return 19;
    if (onepose_mha_softmax(d, 2, d, 0, d, 0, 1, 4, 4, d, 0, nullptr) != ONEPOSE_ERR_INVALID) return 20;
  }
  std::printf("superglue size queries ok (%zu)\n", acc);
  return 0;
}
