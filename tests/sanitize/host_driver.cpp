// Sanitizer driver (test infrastructure): the library's host-only code -- the matcher and
// SuperPoint weight packers, and every workspace / cache size query over a sweep of shapes
// (ragged, tiny, batched, sharded) -- in a host-only -fsanitize=address,undefined build of
// onepose_amd/csrc (no GPU call is made).  Built and run by tests/test_sanitize.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "onepose_hip.h"

namespace {
unsigned s = 2024u;
float frand() {
  s = s * 1664525u + 1013904223u;
  return (float)((s >> 8) / 16777216.0 - 0.5);
}
}  // namespace

int main() {
  if (onepose_abi_version() != 9) return 1;
  // matcher packer
  {
    const int n = onepose_matcher_num_tensors();
    std::vector<std::vector<float>> t(n);
    std::vector<const float*> p(n);
    for (int i = 0; i < n; ++i) {
      if (!onepose_matcher_tensor_name(i)) return 2;
      t[i].resize((size_t)onepose_matcher_tensor_numel(i));
      for (float& x : t[i]) x = frand();
      p[i] = t[i].data();
    }
    std::vector<unsigned char> packed(onepose_matcher_packed_bytes());
    if (onepose_matcher_pack(p.data(), n, packed.data()) != ONEPOSE_OK) return 3;
    // wrong tensor count: must fail cleanly
    if (onepose_matcher_pack(p.data(), n - 1, packed.data()) == ONEPOSE_OK) return 4;
    std::printf("matcher pack: %d tensors, %zu bytes\n", n, packed.size());
  }
  // SuperPoint packer
  {
    // (cin, cout, k) of conv1a .. convDb, the reference's SuperPoint (superpoint.py:147-162)
    const int layers[12][3] = {{1, 64, 3},    {64, 64, 3},   {64, 64, 3},    {64, 64, 3},
                               {64, 128, 3},  {128, 128, 3}, {128, 128, 3},  {128, 128, 3},
                               {128, 256, 3}, {256, 65, 1},  {128, 256, 3},  {256, 256, 1}};
    const int n = onepose_superpoint_num_tensors();
    if (n != 24) return 6;
    std::vector<std::vector<float>> t(n);
    std::vector<const float*> p(n);
    for (int i = 0; i < n; ++i) {
      const int* L = layers[i / 2];
      t[i].resize(i % 2 ? (size_t)L[1] : (size_t)L[1] * L[0] * L[2] * L[2]);
      for (float& x : t[i]) x = frand();
      p[i] = t[i].data();
    }
    std::vector<unsigned char> packed(onepose_superpoint_packed_bytes());
    if (onepose_superpoint_pack(p.data(), n, packed.data()) != ONEPOSE_OK) return 5;
    std::printf("superpoint pack: %d tensors, %zu bytes\n", n, packed.size());
    // the single-layer entry point refuses bad arguments before it launches anything
    const void* pk = packed.data();
    const float* x = t[0].data();
    float* y = t[0].data();
    if (onepose_superpoint_layer(nullptr, 0, x, 1, 2, 2, y, nullptr) != ONEPOSE_ERR_INVALID) return 11;
    if (onepose_superpoint_layer(pk, 0, nullptr, 1, 2, 2, y, nullptr) != ONEPOSE_ERR_INVALID) return 11;
    if (onepose_superpoint_layer(pk, 0, x, 1, 2, 2, nullptr, nullptr) != ONEPOSE_ERR_INVALID) return 11;
    if (onepose_superpoint_layer(pk, -1, x, 1, 2, 2, y, nullptr) != ONEPOSE_ERR_INVALID) return 12;
    if (onepose_superpoint_layer(pk, 12, x, 1, 2, 2, y, nullptr) != ONEPOSE_ERR_INVALID) return 12;
    if (onepose_superpoint_layer(pk, 2, x, 1, 0, 2, y, nullptr) != ONEPOSE_ERR_INVALID) return 13;
    if (onepose_superpoint_layer(pk, 2, x, 1, 2, -4, y, nullptr) != ONEPOSE_ERR_INVALID) return 13;
    if (onepose_superpoint_layer(pk, 2, x, 0, 2, 2, y, nullptr) != ONEPOSE_ERR_INVALID) return 13;
    if (onepose_superpoint_layer(pk, 2, x, 1, 4096, 2048, y, nullptr) != ONEPOSE_ERR_INVALID) return 13;
    if (onepose_superpoint_layer(pk, 2, x, 1, 65536, 65536, y, nullptr) != ONEPOSE_ERR_INVALID) return 13;
    for (int l : {1, 3, 5}) {   // the pooled layers need even sides
      if (onepose_superpoint_layer(pk, l, x, 1, 3, 4, y, nullptr) != ONEPOSE_ERR_INVALID) return 14;
      if (onepose_superpoint_layer(pk, l, x, 1, 4, 5, y, nullptr) != ONEPOSE_ERR_INVALID) return 14;
    }
    if (!onepose_last_error()[0]) return 15;
    // output sizes: plain, pooled, score head; 0 for what the entry point refuses
    if (onepose_superpoint_layer_out_floats(0, 3, 5) != 64u * 15) return 16;
    if (onepose_superpoint_layer_out_floats(5, 4, 6) != 128u * 6) return 16;
    if (onepose_superpoint_layer_out_floats(9, 3, 5) != 64u * 15) return 16;
    if (onepose_superpoint_layer_out_floats(11, 2, 18) != 256u * 36) return 16;
    if (onepose_superpoint_layer_out_floats(12, 2, 2) || onepose_superpoint_layer_out_floats(-1, 2, 2) ||
        onepose_superpoint_layer_out_floats(3, 0, 2) || onepose_superpoint_layer_out_floats(3, 4096, 2048))
      return 17;
  }
  // size queries
  const int shapes[][4] = {{1, 1, 1, 1},     {1, 256, 512, 8},  {2, 1024, 4096, 8},
                           {1, 1024, 2500, 8}, {32, 1024, 16384, 8}, {1, 2048, 8192, 12},
                           {3, 37, 101, 3}};
  size_t acc = 0;
  for (const auto& sh : shapes) {
    const int B = sh[0], n1 = sh[1], n3 = sh[2], L = sh[3];
    acc += onepose_match_workspace_bytes(B, n1, n3, L, 0) + onepose_match_workspace_bytes(B, n1, n3, L, 1);
    acc += onepose_leaves_prepared_bytes(B, n3, L);
    acc += onepose_object_cache_bytes(n3, L, 0) + onepose_object_cache_bytes(n3, L, ONEPOSE_OBJ_GAT_TABLES);
    acc += onepose_object_prepare_workspace_bytes(n3, L);
    for (int prec = 0; prec <= 3; ++prec) {   // (3: refused, 0 bytes)
      acc += onepose_match_workspace_bytes_ex(B, n1, n3, L, 1, prec);
      acc += onepose_object_cache_bytes_ex(n3, L, ONEPOSE_OBJ_GAT_TABLES, prec);
    }
    for (int world = 1; world <= 3; ++world) {
      acc += onepose_match_sharded_xchg_bytes(B, n1, n3, world);
      for (int r = 0; r < world; ++r) acc += onepose_match_sharded_workspace_bytes(B, n1, n3, world, r, L, 1);
    }
    acc += onepose_pnp_workspace_bytes(B, n1, 10000);
    // where each stage leaves the states / final descriptors: inside the workspace, or the cache
    for (int prec = 0; prec <= 2; ++prec) {
      const size_t ws = onepose_match_workspace_bytes_ex(B, n1, n3, L, 1, prec);
      for (int stage = ONEPOSE_STAGE_INPUTS; stage <= ONEPOSE_STAGE_WINNERS; ++stage)
        for (int region = ONEPOSE_REGION_STATE2D; region <= ONEPOSE_REGION_DESC3D; ++region) {
          int where = -1;
          size_t off = 0, bytes = 0;
          const int rc = onepose_match_workspace_region(B, n1, n3, L, 1, prec, region, stage,
                                                        &where, &off, &bytes);
          const bool desc = region >= ONEPOSE_REGION_DESC2D;
          if (desc && stage < ONEPOSE_STAGE_FINAL) {
            if (rc == ONEPOSE_OK) return 7;
            continue;
          }
          if (rc != ONEPOSE_OK || bytes == 0) return 8;
          if (where == ONEPOSE_WHERE_WORKSPACE && off + bytes > ws) return 9;
          acc += off + bytes;
        }
    }
  }
  // the solver's size limit: points of 20 B beside its state in 160 KB of LDS
  const int pnp_max = onepose_pnp_max_points();
  if (pnp_max < 2048 || pnp_max >= 8192) return 10;
  acc += onepose_pnp_workspace_bytes(1, pnp_max, 10000);
  acc += onepose_superpoint_workspace_bytes(1, 512, 512) + onepose_superpoint_detect_workspace_bytes(2, 480, 640);
  std::printf("size queries ok (%zu)\n", acc);
  return 0;
}
