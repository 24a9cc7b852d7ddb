// The matcher's packed weight panel: its layout constants and the accessors matcher.hip reads
// the device copy through.  matcher_pack.hip (host only) writes the panel in this layout.
#pragma once

#include <stdint.h>

namespace onepose {

constexpr int kLayers = 12;
constexpr int kApLayers = 8;
constexpr int kGatLayers = 4;

// packed panel, floats (per attention layer):
//   Wqkv [768][256]: rows 0..255 q head-major (packed row h*64+d <- reference row d*4+h),
//                    then per head h: 64 rows of k_h, 64 rows of v_h
//   bqkv [768]
//   W1a [512][256] = mlp.0.weight[:, :256]
//   C   [512][256] = mlp.0.weight[:, 256:] @ merge.weight, columns head-major (h*64+q)
//   b1f [512]      = mlp.0.bias + mlp.0.weight[:, 256:] @ merge.bias
//   W2 [256][512], b2 [256]
//   CT [4][64][512]: CT[h][q][o] = C[o][h*64+q]  (the fold's operand, o contiguous)
constexpr int64_t kApWqkv = 768 * 256, kApBqkv = 768;
constexpr int64_t kApW1a = 512 * 256, kApC = 512 * 256, kApB1 = 512, kApW2 = 256 * 512,
                  kApB2 = 256, kApCT = 512 * 256;
constexpr int64_t kApFloats = kApWqkv + kApBqkv + kApW1a + kApC + kApB1 + kApW2 + kApB2 + kApCT;
constexpr int64_t kGatFloats = 512;
constexpr int64_t kFinalFloats = 256 * 256 + 256;
constexpr int64_t kPackedFloats = kApLayers * kApFloats + kGatLayers * kGatFloats + kFinalFloats;
// ... then, per attention layer, the bf16 planes of its three weight matrices for the bf16
// modes (gemm.h GemmProb::Wp): Wqkv, W1a and W2 split exactly into hi / mid / lo
// (hi = bf16(x) rounded to nearest even: PM_BF16's operand), [3][rows][cols] uint16 each.
constexpr int64_t kPlWqkv = 768 * 256, kPlW1a = 512 * 256, kPlW2 = 256 * 512;
constexpr int64_t kApPlanes = 3 * (kPlWqkv + kPlW1a + kPlW2);   // uint16 per layer
constexpr int64_t kPackedBytes = kPackedFloats * 4 + kApLayers * kApPlanes * 2;

struct ApW {
  const float *wqkv, *bqkv, *w1a, *c, *b1, *w2, *b2, *ct;
  const uint16_t *wqkv_p, *w1a_p, *w2_p;   // bf16 planes
};
inline ApW ap_weights(const float* base, int ap) {
  const float* p = base + (int64_t)ap * kApFloats;
  ApW w;
  const uint16_t* pl = reinterpret_cast<const uint16_t*>(base + kPackedFloats) + (int64_t)ap * kApPlanes;
  w.wqkv_p = pl;
  w.w1a_p = pl + 3 * kPlWqkv;
  w.w2_p = w.w1a_p + 3 * kPlW1a;
  w.wqkv = p; p += kApWqkv;
  w.bqkv = p; p += kApBqkv;
  w.w1a = p; p += kApW1a;
  w.c = p; p += kApC;
  w.b1 = p; p += kApB1;
  w.w2 = p; p += kApW2;
  w.b2 = p; p += kApB2;
  w.ct = p;
  return w;
}
inline const float* gat_weights(const float* base, int g) {
  return base + kApLayers * kApFloats + (int64_t)g * kGatFloats;
}
inline const float* final_weights(const float* base) {
  return base + kApLayers * kApFloats + kGatLayers * kGatFloats;
}

}  // namespace onepose
