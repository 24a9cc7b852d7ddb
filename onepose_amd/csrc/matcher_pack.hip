// Host-only weight packer of the GATsSPG matcher: the reference state dict's tensors ->
// the packed panel of matcher_pack.h (onepose_matcher_pack and the tensor name / size queries).
// No kernels and no device call: this is the code the host sanitizer driver exercises.
#include <cstring>
#include <vector>

#include "common.h"
#include "matcher_pack.h"

namespace onepose {
namespace {

// bf16 bits of x rounded to nearest even (the device's (__bf16)x for finite x)
uint16_t bf16_rne(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
float bf16_val(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
// the exact split x = hi + mid + lo of gemm.hip's store_quad_bf16, into planes n elements apart
void split_planes(const float* x, int64_t n, uint16_t* out) {
  for (int64_t i = 0; i < n; ++i) {
    const uint16_t h = bf16_rne(x[i]);
    const float r = x[i] - bf16_val(h);
    const uint16_t m = bf16_rne(r);
    out[i] = h;
    out[n + i] = m;
    out[2 * n + i] = bf16_rne(r - bf16_val(m));
  }
}

struct TensorSpec {
  std::string name;
  int64_t numel;
};

const std::vector<TensorSpec>& tensor_specs() {
  static std::vector<TensorSpec> specs = [] {
    std::vector<TensorSpec> s;
    for (int i = 0; i < kLayers; ++i) {
      std::string p = "gnn.layers." + std::to_string(i) + ".";
      if (i % 3 == 0) {
        s.push_back({p + "W", 256 * 256});
        s.push_back({p + "a", 512});
      } else {
        for (int j = 0; j < 3; ++j) {
          s.push_back({p + "attn.proj." + std::to_string(j) + ".weight", 256 * 256});
          s.push_back({p + "attn.proj." + std::to_string(j) + ".bias", 256});
        }
        s.push_back({p + "attn.merge.weight", 256 * 256});
        s.push_back({p + "attn.merge.bias", 256});
        s.push_back({p + "mlp.0.weight", 512 * 512});
        s.push_back({p + "mlp.0.bias", 512});
        s.push_back({p + "mlp.3.weight", 256 * 512});
        s.push_back({p + "mlp.3.bias", 256});
      }
    }
    s.push_back({"final_proj.weight", 256 * 256});
    s.push_back({"final_proj.bias", 256});
    return s;
  }();
  return specs;
}

}  // namespace
}  // namespace onepose

using namespace onepose;

extern "C" {

int onepose_matcher_num_tensors(void) { return (int)tensor_specs().size(); }

const char* onepose_matcher_tensor_name(int i) {
  const auto& s = tensor_specs();
  if (i < 0 || i >= (int)s.size()) return nullptr;
  return s[i].name.c_str();
}

int64_t onepose_matcher_tensor_numel(int i) {
  const auto& s = tensor_specs();
  if (i < 0 || i >= (int)s.size()) return -1;
  return s[i].numel;
}

size_t onepose_matcher_packed_bytes(void) { return (size_t)kPackedBytes; }

int onepose_matcher_pack(const float* const* tensors, int n_tensors, void* packed_host) {
  clear_error();
  const auto& specs = tensor_specs();
  OP_REQUIRE(tensors != nullptr && packed_host != nullptr, "pack: null pointer");
  OP_REQUIRE(n_tensors == (int)specs.size(), "pack: expected %d tensors, got %d",
             (int)specs.size(), n_tensors);
  for (int i = 0; i < n_tensors; ++i) OP_REQUIRE(tensors[i] != nullptr, "pack: tensor %d null", i);
  float* out = static_cast<float*>(packed_host);
  int ti = 0, ap = 0, gat = 0;
  for (int layer = 0; layer < kLayers; ++layer) {
    if (layer % 3 == 0) {
      const float* W = tensors[ti++];   // [256 in][256 out]
      const float* a = tensors[ti++];   // [512]
      float* wa = out + kApLayers * kApFloats + (int64_t)gat * kGatFloats;
      for (int c = 0; c < 256; ++c) {
        double lo = 0.0, hi = 0.0;
        for (int j = 0; j < 256; ++j) {
          lo += (double)W[c * 256 + j] * (double)a[j];
          hi += (double)W[c * 256 + j] * (double)a[256 + j];
        }
        wa[c] = (float)lo;
        wa[256 + c] = (float)hi;
      }
      ++gat;
      continue;
    }
    float* p = out + (int64_t)ap * kApFloats;
    float* wq = p;
    float* wkv = wq + 256 * 256;
    float* bq = p + kApWqkv;
    float* bkv = bq + 256;
    float* w1a = bq + kApBqkv;
    float* cw = w1a + kApW1a;
    float* b1 = cw + kApC;
    float* w2 = b1 + kApB1;
    float* b2 = w2 + kApW2;
    const float* pw[3];
    const float* pb[3];
    for (int j = 0; j < 3; ++j) {
      pw[j] = tensors[ti++];
      pb[j] = tensors[ti++];
    }
    const float* mw = tensors[ti++];   // merge [256][256]
    const float* mb = tensors[ti++];
    const float* m0w = tensors[ti++];  // mlp.0 [512][512]
    const float* m0b = tensors[ti++];
    const float* m3w = tensors[ti++];  // mlp.3 [256][512]
    const float* m3b = tensors[ti++];
    // q: packed row h*64+d <- reference row d*4+h (view(B, 64, 4, N), :116)
    for (int cp = 0; cp < 256; ++cp) {
      const int h = cp / 64, d = cp % 64, cr = d * 4 + h;
      memcpy(wq + (int64_t)cp * 256, pw[0] + (int64_t)cr * 256, 256 * sizeof(float));
      bq[cp] = pb[0][cr];
    }
    // k / v interleaved per head: rows [128h, 128h+64) = k_h, [128h+64, 128h+128) = v_h
    for (int h = 0; h < 4; ++h)
      for (int d = 0; d < 64; ++d) {
        const int cr = d * 4 + h;
        memcpy(wkv + (int64_t)(128 * h + d) * 256, pw[1] + (int64_t)cr * 256, 256 * sizeof(float));
        memcpy(wkv + (int64_t)(128 * h + 64 + d) * 256, pw[2] + (int64_t)cr * 256,
               256 * sizeof(float));
        bkv[128 * h + d] = pb[1][cr];
        bkv[128 * h + 64 + d] = pb[2][cr];
      }
    // MLP conv 1 split: x part as is; message part folded with the merge conv.  Each output is
    // one double chain over j in ascending order; the merge weight is read through a
    // transposed double copy (packed column order) and eight chains run side by side, so the
    // fold is not bound by strided loads and one dependent chain (1.09 -> 0.19 s per model on
    // this container's CPU; the same chains, the same bits).
    std::vector<double> mwt((size_t)256 * 256);   // [cp][j] = merge[j][cr(cp)]
    for (int cp = 0; cp < 256; ++cp) {   // merge input channel q*4+h -> packed h*64+q
      const int h = cp / 64, q = cp % 64, cr = q * 4 + h;
      for (int j = 0; j < 256; ++j) mwt[(size_t)cp * 256 + j] = (double)mw[(int64_t)j * 256 + cr];
    }
    for (int o = 0; o < 512; ++o) {
      memcpy(w1a + (int64_t)o * 256, m0w + (int64_t)o * 512, 256 * sizeof(float));
      const float* mo = m0w + (int64_t)o * 512 + 256;
      double bacc = (double)m0b[o];
      for (int j = 0; j < 256; ++j) bacc += (double)mo[j] * mb[j];
      b1[o] = (float)bacc;
      double arow[256];
      for (int j = 0; j < 256; ++j) arow[j] = (double)mo[j];
      for (int cp0 = 0; cp0 < 256; cp0 += 8) {
        double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const double* wt = mwt.data() + (size_t)cp0 * 256;
        for (int j = 0; j < 256; ++j)
          for (int k = 0; k < 8; ++k) acc[k] += arow[j] * wt[(size_t)k * 256 + j];
        for (int k = 0; k < 8; ++k) cw[(int64_t)o * 256 + cp0 + k] = (float)acc[k];
      }
    }
    memcpy(w2, m3w, kApW2 * sizeof(float));
    memcpy(b2, m3b, kApB2 * sizeof(float));
    float* ct = b2 + kApB2;
    for (int o = 0; o < 512; ++o)
      for (int cp = 0; cp < 256; ++cp) ct[(int64_t)cp * 512 + o] = cw[(int64_t)o * 256 + cp];
    uint16_t* pl = reinterpret_cast<uint16_t*>(out + kPackedFloats) + (int64_t)ap * kApPlanes;
    split_planes(wq, kPlWqkv, pl);   // wq: the whole [768][256] panel (q rows, then k_h / v_h)
    split_planes(w1a, kPlW1a, pl + 3 * kPlWqkv);
    split_planes(w2, kPlW2, pl + 3 * (kPlWqkv + kPlW1a));
    ++ap;
  }
  float* fin = out + kApLayers * kApFloats + kGatLayers * kGatFloats;
  memcpy(fin, tensors[ti++], 256 * 256 * sizeof(float));
  memcpy(fin + 256 * 256, tensors[ti++], 256 * sizeof(float));
  return ONEPOSE_OK;
}

}  // extern "C"
