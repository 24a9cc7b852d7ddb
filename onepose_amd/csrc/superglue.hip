// SuperGlue 2D-2D matcher forward on gfx950 (src/models/matchers/SuperGlue/superglue.py:50-327),
// fp32.  The 1x1 convolutions are the token GEMM (gemm.h) as it stands; new here are the
// multi-head softmax attention and the log-domain optimal transport (Sinkhorn).
//
// Data layout in the workspace (per batch sample, fp32, token-major like the GATsSPG matcher):
//   X[2][side] [n][256]     descriptor state, ping-pong
//   QKV[side]  [n][768]     [q | k | v], each 4 heads x 64, head-major channels (h*64 + d)
//   MSG[side]  [n][256]     attention output, head-major (the merge conv is folded into MLP conv 1)
//   Y1[side]   [n][512]     MLP hidden (eval BatchNorm folded into conv 1; ReLU in conv 2's prologue)
//   S          [n0][ldS]    scores mdesc0 . mdesc1 / 16, ldS = n1 rounded up to 4
//   u [n0+1], v [n1+1]      Sinkhorn potentials (float64); the couplings [[S, a], [a, a]] are never built:
//                           the dustbin row and column are the constant bin_score
// One layer (AttentionalPropagation, :150-159), both images in every launch:
//   1. QKV GEMM (EPI_BIAS, N = 768)      2. softmax attention (self: own k/v, cross: the other's)
//   3. MLP conv 1 on cat[x, msg] (EPI_BIAS, A0/A1 split at 256; [W1a | W1b Wm], BN folded)
//   4. MLP conv 2 on ReLU(.) + residual (EPI_RESID, PRO_NORM_RELU with mean 0 / rstd 1: (a-0)*1
//      is exact, so the prologue is a plain ReLU)
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gemm.h"

namespace onepose {
namespace {

constexpr int kSgLayers = 18;        // ['self', 'cross'] * 9 (superglue.py:242)
constexpr int kSgMaxPoints = 16384;  // per image
constexpr double kBnEps = 1e-5;      // nn.BatchNorm1d default

// ------------------------------------------------------------------------------------
// packed panel (floats)
// ------------------------------------------------------------------------------------
// keypoint encoder [3, 32, 64, 128, 256, 256] (eval BatchNorm folded into each conv but the last):
//   W1t [3][32], b1 [32], W2t [32][64], b2 [64], W3t [64][128], b3 [128]   (in-major: the small
//                                                                          kernel's lanes are outputs)
//   W4 [256][128], b4 [256], W5 [256][256], b5 [256]                       (out-major: token GEMM)
//   zeros [512], ones [512]: the mean / rstd that make PRO_NORM_RELU a plain ReLU
constexpr int64_t kKeW1 = 0, kKeB1 = kKeW1 + 96, kKeW2 = kKeB1 + 32, kKeB2 = kKeW2 + 2048,
                  kKeW3 = kKeB2 + 64, kKeB3 = kKeW3 + 8192, kKeW4 = kKeB3 + 128,
                  kKeB4 = kKeW4 + 256 * 128, kKeW5 = kKeB4 + 256, kKeB5 = kKeW5 + 65536,
                  kKeZeros = kKeB5 + 256, kKeOnes = kKeZeros + 512, kKeFloats = kKeOnes + 512;
// per layer:
//   Wqkv [768][256]: rows 0..255 q, 256..511 k, 512..767 v, each head-major (packed row h*64+d
//                    <- reference row d*4+h: .view(B, 64, 4, N) makes channel c = d*4 + h)
//   bqkv [768]
//   W1f [512][512] = s * [mlp.0.weight[:, :256] | mlp.0.weight[:, 256:] @ merge.weight], the
//                    message columns head-major; s = gamma / sqrt(var + eps) of mlp.1
//   b1f [512]      = s * (mlp.0.bias + mlp.0.weight[:, 256:] @ merge.bias - mean) + beta
//   W2 [256][512], b2 [256]
constexpr int64_t kLyWqkv = 0, kLyBqkv = kLyWqkv + 768 * 256, kLyW1 = kLyBqkv + 768,
                  kLyB1 = kLyW1 + 512 * 512, kLyW2 = kLyB1 + 512, kLyB2 = kLyW2 + 256 * 512,
                  kLyFloats = kLyB2 + 256;
// then final_proj [256][256] + [256], then bin_score (one float, padded to 64)
constexpr int64_t kSgLayer0 = kKeFloats, kSgFinal = kSgLayer0 + kSgLayers * kLyFloats,
                  kSgBin = kSgFinal + 65536 + 256, kSgFloats = kSgBin + 64;

struct SgSpec {
  std::string name;
  int64_t numel;
};
constexpr int kEncCh[6] = {3, 32, 64, 128, 256, 256};

const std::vector<SgSpec>& sg_specs() {
  static std::vector<SgSpec> specs = [] {
    std::vector<SgSpec> s;
    s.push_back({"bin_score", 1});
    for (int i = 0; i < 5; ++i) {
      const std::string c = "kenc.encoder." + std::to_string(3 * i) + ".";
      s.push_back({c + "weight", (int64_t)kEncCh[i + 1] * kEncCh[i]});
      s.push_back({c + "bias", kEncCh[i + 1]});
      if (i < 4) {
        const std::string b = "kenc.encoder." + std::to_string(3 * i + 1) + ".";
        for (const char* k : {"weight", "bias", "running_mean", "running_var"})
          s.push_back({b + k, kEncCh[i + 1]});
      }
    }
    for (int l = 0; l < kSgLayers; ++l) {
      const std::string p = "gnn.layers." + std::to_string(l) + ".";
      s.push_back({p + "attn.merge.weight", 65536});
      s.push_back({p + "attn.merge.bias", 256});
      for (int j = 0; j < 3; ++j) {
        s.push_back({p + "attn.proj." + std::to_string(j) + ".weight", 65536});
        s.push_back({p + "attn.proj." + std::to_string(j) + ".bias", 256});
      }
      s.push_back({p + "mlp.0.weight", 512 * 512});
      s.push_back({p + "mlp.0.bias", 512});
      for (const char* k : {"weight", "bias", "running_mean", "running_var"})
        s.push_back({p + "mlp.1." + k, 512});
      s.push_back({p + "mlp.3.weight", 256 * 512});
      s.push_back({p + "mlp.3.bias", 256});
    }
    s.push_back({"final_proj.weight", 65536});
    s.push_back({"final_proj.bias", 256});
    return s;
  }();
  return specs;
}

// ------------------------------------------------------------------------------------
// input stage
// ------------------------------------------------------------------------------------
struct SgSideIn {
  const float* desc;   // [B][256][n]
  const float* kpts;   // [B][n][2]
  const float* scores; // [B][n]
  int64_t desc_bs, kpts_bs, scores_bs;   // elements; 0 = shared by the batch
  int n;
  float cx, cy, scale;   // normalize_keypoints: centre (w/2, h/2), 0.7 * max(w, h)
  const int* counts;     // counts entries: [B] real tokens per sample, or null (all n)
  const int* hw;         // counts entries: [B][2] (h, w) per sample, or null (cx, cy, scale above)
  float* xd;   // [B][n][256] descriptors, token-major
  float* h3;   // [B][n][128] encoder layer 3 output after ReLU
  int tiles;   // workgroups per sample of the kernel at hand
};
struct SgInArgs {
  SgSideIn p[2];
  int batch;
};

// A sample's own token count in the entries that take counts: read on the device, clamped to
// [0, n]; a null array is "every sample has n".  Every kernel below has a CNT = false
// instantiation, which the uniform entries launch and which never looks at the arrays, and a
// CNT = true one for the counts entries, where n (m) of sample b comes from here while the
// strides and the grid stay those of the batch maxima.
__device__ __forceinline__ int sg_count(const int* counts, int b, int n) {
  if (counts == nullptr) return n;
  const int c = counts[b];
  return c < 0 ? 0 : (c > n ? n : c);
}

// [B][256][n] -> [B][n][256], 64 tokens x 64 channels per workgroup through a padded LDS tile.
// CNT: tokens past the sample's count are written as zero rows.
template <bool CNT>
__global__ __launch_bounds__(256) void sg_transpose_kernel(SgInArgs args) {
  __shared__ float tile[64][65];
  int bid = blockIdx.x;
  const bool second = bid >= args.p[0].tiles * args.batch;
  const SgSideIn& P = second ? args.p[1] : args.p[0];
  if (second) bid -= args.p[0].tiles * args.batch;
  const int b = bid / P.tiles, r = bid - b * P.tiles;
  const int n0 = (r >> 2) * 64, c0 = (r & 3) * 64, n = P.n;
  const int nb = CNT ? sg_count(P.counts, b, n) : n;
  const float* s = P.desc + (int64_t)b * P.desc_bs;
  const int t = threadIdx.x;
  for (int i = 0; i < 16; ++i) {
    const int ch = (t >> 6) + 4 * i, tk = t & 63;
    tile[ch][tk] = (n0 + tk < nb) ? s[(int64_t)(c0 + ch) * n + n0 + tk] : 0.f;
  }
  __syncthreads();
  float* d = P.xd + (int64_t)b * n * kDim;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int e = t + 256 * i, tk = e >> 4, cq = (e & 15) * 4;
    if (n0 + tk < n)
      *reinterpret_cast<float4*>(d + (int64_t)(n0 + tk) * kDim + c0 + cq) =
          make_float4(tile[cq][tk], tile[cq + 1][tk], tile[cq + 2][tk], tile[cq + 3][tk]);
  }
}

// normalize_keypoints + the encoder's first three layers (3 -> 32 -> 64 -> 128, BatchNorm folded,
// ReLU), eight tokens per workgroup: a thread owns one output channel of all eight, so a weight
// is loaded once per eight FMAs.  Layers 4 and 5 (K = 128, 256) are token GEMMs.
// CNT: centre and scale from the sample's own (h, w) (values below 1 read as 1), and zero rows past
// the sample's count.
constexpr int kKencTok = 8;
template <bool CNT>
__global__ __launch_bounds__(128) void sg_kenc_kernel(SgInArgs args, const float* __restrict__ w) {
  __shared__ float in[kKencTok][4], h1[kKencTok][32], h2[kKencTok][64];
  int bid = blockIdx.x;
  const bool second = bid >= args.p[0].tiles * args.batch;
  const SgSideIn& P = second ? args.p[1] : args.p[0];
  if (second) bid -= args.p[0].tiles * args.batch;
  const int b = bid / P.tiles, t0 = (bid - b * P.tiles) * kKencTok, t = threadIdx.x;
  const int nb = CNT ? sg_count(P.counts, b, P.n) : P.n;
  if (t < kKencTok) {
    const int tok = t0 + t;
    float x = 0.f, y = 0.f, sc = 0.f;
    if (tok < nb) {
      float cx = P.cx, cy = P.cy, scale = P.scale;
      if (CNT && P.hw != nullptr) {   // the host's arithmetic (sg_forward), per sample
        const int hi = P.hw[2 * b], wi = P.hw[2 * b + 1];
        const float h = (float)(hi < 1 ? 1 : hi), w = (float)(wi < 1 ? 1 : wi);
        cx = w / 2.f;
        cy = h / 2.f;
        scale = (w > h ? w : h) * 0.7f;
      }
      const float* kp = P.kpts + (int64_t)b * P.kpts_bs + (int64_t)tok * 2;
      x = (kp[0] - cx) / scale;
      y = (kp[1] - cy) / scale;
      sc = P.scores[(int64_t)b * P.scores_bs + tok];
    }
    in[t][0] = x;
    in[t][1] = y;
    in[t][2] = sc;
  }
  __syncthreads();
  if (t < 32) {
    const float w0 = w[kKeW1 + t], w1 = w[kKeW1 + 32 + t], w2 = w[kKeW1 + 64 + t], bb = w[kKeB1 + t];
#pragma unroll
    for (int k = 0; k < kKencTok; ++k)
      h1[k][t] = fmaxf(fmaf(w2, in[k][2], fmaf(w1, in[k][1], fmaf(w0, in[k][0], bb))), 0.f);
  }
  __syncthreads();
  if (t < 64) {
    float acc[kKencTok];
    const float bb = w[kKeB2 + t];
#pragma unroll
    for (int k = 0; k < kKencTok; ++k) acc[k] = bb;
    for (int c = 0; c < 32; ++c) {
      const float wv = w[kKeW2 + c * 64 + t];
#pragma unroll
      for (int k = 0; k < kKencTok; ++k) acc[k] = fmaf(wv, h1[k][c], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < kKencTok; ++k) h2[k][t] = fmaxf(acc[k], 0.f);
  }
  __syncthreads();
  {
    float acc[kKencTok];
    const float bb = w[kKeB3 + t];
#pragma unroll
    for (int k = 0; k < kKencTok; ++k) acc[k] = bb;
    for (int c = 0; c < 64; ++c) {
      const float wv = w[kKeW3 + c * 128 + t];
#pragma unroll
      for (int k = 0; k < kKencTok; ++k) acc[k] = fmaf(wv, h2[k][c], acc[k]);
    }
    float* o = P.h3 + ((int64_t)b * P.n + t0) * 128 + t;
#pragma unroll
    for (int k = 0; k < kKencTok; ++k)
      if (t0 + k < P.n) o[(int64_t)k * 128] = (!CNT || t0 + k < nb) ? fmaxf(acc[k], 0.f) : 0.f;
  }
}

// ------------------------------------------------------------------------------------
// multi-head softmax attention: out = softmax(q k^T / 8) v per head (superglue.py:103-119)
// ------------------------------------------------------------------------------------
// A wave owns 32 queries of one (sample, head) over all keys; a workgroup of NW waves shares the
// K / V tiles (64 keys) staged in LDS.  Per 32-key block the wave computes the TRANSPOSED score
// tile St[key][query] = sum_d K[key][d] (Q[query][d] / 8) on v_mfma_f32_32x32x2_f32 (A = K from
// LDS, B = Q held in 32 registers; /8 is exact), so each lane owns one query column: 16 keys in
// its accumulator registers, the other 16 in lane ^ 32.  The running max / sum are register
// reductions plus one exchange across the halves, and the probabilities feed the second MFMA
// Ot[d][query] += V[key][d] P[key][query] as its B operand straight from the accumulator
// registers: accumulator register r of half hh holds key 8 (r / 4) + 4 hh + r % 4, and an MFMA
// step contracts one key per half, so step r takes exactly those two keys (A = V rows from LDS).
// The contraction order over d (half hh takes d = 32 hh + s at step s) and over keys is free.
// Keys past m are masked to -inf before the max (weight exactly 0) and their LDS rows are zero;
// queries past n load zeros and are not stored.  No workgroup waits for another.
struct AttnProb {
  const float *q, *k, *v;
  float* o;
  int64_t q_bs, k_bs, v_bs, o_bs;   // per sample, elements
  int ldq, ldk, ldv, ldo;           // row strides, elements (multiples of 4)
  int n, m;                         // queries, keys
  int qtiles;                       // ceil(n / (32 NW))
  const int *counts_q, *counts_k;   // counts entries: [B] real queries / keys, or null (n / m)
};
struct AttnArgs {
  AttnProb p[2];
  int batch;
};
constexpr int kAttnKT = 64, kAttnKP = 68;   // keys per tile, K row pitch (16-B aligned rows)
__device__ __forceinline__ int ceil_div_dev(int a, int b) { return (a + b - 1) / b; }

// KS = 1: the NW waves of a workgroup own 32 queries each and share one staged tile.  KS = 4
// (NW = 1; small problems, where 32-query tiles alone leave most SIMDs idle): the four waves own
// the SAME 32 queries and every fourth key tile each, staged in a private LDS region per wave;
// their (max, sum, O) states are merged through LDS in wave order at the end, a fixed order.
//
// CNT: n and m are sample b's own counts.  b is fixed per workgroup, so the trip count (from m)
// and with it every barrier stays uniform within the workgroup; a wave whose queries all lie past
// the sample's n stages tiles and meets the barriers like the others.  Query rows from the
// sample's n up to the batch's n are written as zeros, and so is every row of a sample without
// keys (its sum is 0; nothing is divided by it).  With KS = 4 a short sample leaves waves without
// a key tile: their max stays -inf and the merge skips them, per sample as before per launch.
constexpr int kAttnTileFloats = kAttnKT * kAttnKP + kAttnKT * 64;

template <int NW, int KS, bool CNT>
__global__ __launch_bounds__(NW * KS * 64) void mha_softmax_kernel(AttnArgs args) {
  typedef float floatx16 __attribute__((ext_vector_type(16)));
  extern __shared__ __attribute__((aligned(16))) float attn_lds[];
  constexpr int NT = NW * KS * 64;
  int bid = blockIdx.x;
  const int per0 = args.p[0].qtiles * kHeads * args.batch;
  const bool second = bid >= per0;
  const AttnProb& P = second ? args.p[1] : args.p[0];
  if (second) bid -= per0;
  const int qt = bid % P.qtiles, h = (bid / P.qtiles) % kHeads, b = bid / (P.qtiles * kHeads);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, hh = lane >> 5, l31 = lane & 31;
  const int wq = KS > 1 ? 0 : w, ks = KS > 1 ? w : 0;
  float* Ks = attn_lds + (KS > 1 ? w * kAttnTileFloats : 0);
  float* Vs = Ks + kAttnKT * kAttnKP;
  const int n = CNT ? sg_count(P.counts_q, b, P.n) : P.n;
  const int m = CNT ? sg_count(P.counts_k, b, P.m) : P.m;
  const int q0 = (qt * NW + wq) * 32, query = q0 + l31;
  const bool active = q0 < n;   // wave-uniform

  // Q / 8 for d = 32 hh + s, s = 0..31
  float qr[32];
  {
    const float* qp = P.q + (int64_t)b * P.q_bs + (int64_t)query * P.ldq + h * 64 + hh * 32;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (query < n) x = *reinterpret_cast<const float4*>(qp + 4 * i);
      qr[4 * i] = x.x * 0.125f;
      qr[4 * i + 1] = x.y * 0.125f;
      qr[4 * i + 2] = x.z * 0.125f;
      qr[4 * i + 3] = x.w * 0.125f;
    }
  }
  floatx16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) o0[r] = o1[r] = 0.f;
  float mrun = -INFINITY, lsum = 0.f;

  const float* kg = P.k + (int64_t)b * P.k_bs + h * 64;
  const float* vg = P.v + (int64_t)b * P.v_bs + h * 64;
  const int ntiles = ceil_div_dev(m, kAttnKT), trips = ceil_div_dev(ntiles, KS);
  for (int it = 0; it < trips; ++it) {
    const int k0 = (it * KS + ks) * kAttnKT;   // (KS > 1: may lie past m in the last trip)
    __syncthreads();   // the previous tile's readers are done
    for (int idx = KS > 1 ? lane : t; idx < kAttnKT * 16; idx += KS > 1 ? 64 : NT) {
      const int key = idx >> 4, c4 = (idx & 15) * 4, gk = k0 + key;
      float4 kx = make_float4(0.f, 0.f, 0.f, 0.f), vx = kx;
      if (gk < m) {
        kx = *reinterpret_cast<const float4*>(kg + (int64_t)gk * P.ldk + c4);
        vx = *reinterpret_cast<const float4*>(vg + (int64_t)gk * P.ldv + c4);
      }
      *reinterpret_cast<float4*>(Ks + key * kAttnKP + c4) = kx;
      *reinterpret_cast<float4*>(Vs + key * 64 + c4) = vx;
    }
    __syncthreads();
    if (!active || k0 >= m) continue;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int kb = k0 + sub * 32;   // first key of the 32-key block
      if (kb >= m) break;             // wave-uniform: the block has at least one key below
      floatx16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
      const float* kp = Ks + (sub * 32 + l31) * kAttnKP + hh * 32;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float4 a = *reinterpret_cast<const float4*>(kp + 4 * i);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, qr[4 * i], s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, qr[4 * i + 1], s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, qr[4 * i + 2], s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, qr[4 * i + 3], s, 0, 0, 0);
      }
      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kb + 8 * (r >> 2) + 4 * hh + (r & 3);
        if (key >= m) s[r] = -INFINITY;   // padded key: weight 0
        tmax = fmaxf(tmax, s[r]);
      }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
      const float mnew = fmaxf(mrun, tmax);   // finite: key kb is valid for every query
      const float corr = expf(mrun - mnew);   // 0 on the first block (mrun = -inf)
      lsum *= corr;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        o0[r] *= corr;
        o1[r] *= corr;
      }
      const float* vp = Vs + (sub * 32 + 4 * hh) * 64 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = expf(s[r] - mnew);
        lsum += p;
        const float* vr = vp + (8 * (r >> 2) + (r & 3)) * 64;
        o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[0], p, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[32], p, o1, 0, 0, 0);
      }
      mrun = mnew;
    }
  }
  float ltot = lsum + __shfl_xor(lsum, 32, 64);
  if (KS > 1) {
    // waves 1..KS-1 leave (max, sum, O) in their own regions; wave 0 folds them in, in order
    __syncthreads();   // every wave is done reading its tiles
    if (w > 0) {
      Ks[lane] = mrun;
      Ks[64 + lane] = ltot;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        Ks[(2 + r) * 64 + lane] = o0[r];
        Ks[(18 + r) * 64 + lane] = o1[r];
      }
    }
    __syncthreads();
    if (w > 0) return;
    for (int q = 1; q < KS; ++q) {
      const float* R = attn_lds + q * kAttnTileFloats;
      const float mk = R[lane];
      if (mk == -INFINITY) continue;   // that wave had no keys (wave-uniform: m is)
      const float M = fmaxf(mrun, mk), ca = expf(mrun - M), cb = expf(mk - M);
      ltot = ltot * ca + R[64 + lane] * cb;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        o0[r] = o0[r] * ca + R[(2 + r) * 64 + lane] * cb;
        o1[r] = o1[r] * ca + R[(18 + r) * 64 + lane] * cb;
      }
      mrun = M;
    }
  }
  float* op = P.o + (int64_t)b * P.o_bs + (int64_t)query * P.ldo + h * 64 + 4 * hh;
  if (CNT) {
    if (query >= P.n) return;
    if (query >= n || m == 0) {   // a padded query row, or a sample without keys
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        *reinterpret_cast<float4*>(op + 8 * g) = z;
        *reinterpret_cast<float4*>(op + 32 + 8 * g) = z;
      }
      return;
    }
  } else {
    if (!active) return;
    if (query >= n) return;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    *reinterpret_cast<float4*>(op + 8 * g) = make_float4(
        o0[4 * g] / ltot, o0[4 * g + 1] / ltot, o0[4 * g + 2] / ltot, o0[4 * g + 3] / ltot);
    *reinterpret_cast<float4*>(op + 32 + 8 * g) = make_float4(
        o1[4 * g] / ltot, o1[4 * g + 1] / ltot, o1[4 * g + 2] / ltot, o1[4 * g + 3] / ltot);
  }
}

template <bool CNT>
int attn_launch(AttnArgs& a, int nprob, hipStream_t st) {
  constexpr size_t kTileBytes = (size_t)kAttnTileFloats * 4;
  // small problems (32-query tiles give at most two waves per CU, and there are key tiles to
  // share out): four waves per query tile, each over a quarter of the key tiles
  int64_t wgs1 = 0;
  bool deep = true;
  for (int i = 0; i < nprob; ++i) {
    wgs1 += (int64_t)ceil_div(a.p[i].n, 32) * kHeads * a.batch;
    deep = deep && a.p[i].m >= 2 * kAttnKT;
  }
  const bool split = deep && wgs1 <= 512;
  // otherwise waves per workgroup: as many (4, 2, 1) as still leave a workgroup per CU
  int nw = split ? 1 : 4;
  for (; nw > 1; nw >>= 1) {
    int64_t wgs = 0;
    for (int i = 0; i < nprob; ++i) wgs += (int64_t)ceil_div(a.p[i].n, 32 * nw) * kHeads * a.batch;
    if (wgs >= 256) break;
  }
  int64_t grid = 0;
  for (int i = 0; i < 2; ++i) {
    a.p[i].qtiles = i < nprob ? ceil_div(a.p[i].n, 32 * nw) : 0;
    grid += (int64_t)a.p[i].qtiles * kHeads * a.batch;
  }
  OP_REQUIRE(grid > 0 && grid < (1ll << 31), "mha_softmax: grid of %lld workgroups", (long long)grid);
  if (split) {
    static bool attr_set = false;   // (one per instantiation of this function)
    if (!attr_set) {
      OP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mha_softmax_kernel<1, 4, CNT>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4 * kTileBytes)));
      attr_set = true;
    }
    OP_LAUNCH(K_SG_ATTN, st, (mha_softmax_kernel<1, 4, CNT>), dim3((unsigned)grid), dim3(256),
              4 * kTileBytes, st, a);
  } else if (nw == 4) {
    OP_LAUNCH(K_SG_ATTN, st, (mha_softmax_kernel<4, 1, CNT>), dim3((unsigned)grid), dim3(256), kTileBytes,
              st, a);
  } else if (nw == 2) {
    OP_LAUNCH(K_SG_ATTN, st, (mha_softmax_kernel<2, 1, CNT>), dim3((unsigned)grid), dim3(128), kTileBytes,
              st, a);
  } else {
    OP_LAUNCH(K_SG_ATTN, st, (mha_softmax_kernel<1, 1, CNT>), dim3((unsigned)grid), dim3(64), kTileBytes,
              st, a);
  }
  return ONEPOSE_OK;
}

// ------------------------------------------------------------------------------------
// log-domain optimal transport (superglue.py:181-210)
// ------------------------------------------------------------------------------------
// Z = [[S, a], [a, a]] is (m+1) x (n+1) with a = bin_score; only S is in memory.  Per iteration
//   u_i = log_mu_i - LSE_j(Z_ij + v_j)     row pass: a wave per row, 16-B loads along the row
//   v_j = log_nu_j - LSE_i(Z_ij + u_i)     column pass: a lane per column (coalesced across
//                                          columns), rows in chunks of kSkRows whose (max, sum)
//                                          partials a small kernel merges in chunk order
// Every LSE is max-shifted: a running (max, sum exp(x - max)) per lane, one exp per element.
// All merges (lanes by butterfly, waves and chunks in index order) have a fixed order, and there
// are no atomics, so the result is the same bits on every run.  Plain launches only.
constexpr int kSkRows = 128;   // rows per column-pass chunk

// The potentials u, v (and every LSE's running max and sum) are float64; the matrix and the exps
// are fp32.  With fp32 potentials of magnitude 32..64 (scores of that size are absorbed by them)
// a potential alone is quantised to 4e-6, twenty times the error the exps contribute; in float64
// Z + u + v - norm is rounded to fp32 once, at the end.  The potentials are n + m + 2 numbers, so
// this costs no bandwidth, and the per-element float64 work is two adds and an fma.
struct SkArgs {
  const float* S;
  int64_t s_bs;
  int ld, m, n;
  const float* alpha_p;   // device bin_score, or null: alpha_v
  float alpha_v;
  double* u;              // [B][m+1]
  double* v;              // [B][n+1+pad]
  int64_t v_bs;
  double2* part;          // [B][chunks][n+1] column-pass partials
  int chunks, rows;       // column-pass chunks and rows per chunk (one chunk: all rows)
  double norm, log_mu_bin, log_nu_bin;
  const int *counts_m, *counts_n;   // counts entries: [B] real rows / columns, or null (m / n)
};

// One sample's problem inside the padded layout (the CNT = true kernels): its own m x n, and
// norm / log_mu_bin / log_nu_bin of those in float64 on the device.  The strides (u, v, the
// partials, the outputs) and the chunking stay those of A.m and A.n, the batch maxima.  A sample
// with m = 0 or n = 0 has no transport problem: every kernel leaves it at once (b is fixed per
// workgroup, so no barrier is split) and sg_mutual_kernel writes its "no match" rows.
struct SkDims {
  int m, n;
  bool empty;
};
template <bool CNT>
__device__ __forceinline__ SkDims sk_dims(const SkArgs& A, int b) {
  SkDims d{A.m, A.n, false};
  if (CNT) {
    d.m = sg_count(A.counts_m, b, A.m);
    d.n = sg_count(A.counts_n, b, A.n);
    d.empty = d.m == 0 || d.n == 0;
  }
  return d;
}
template <bool CNT>
__device__ __forceinline__ double sk_norm(const SkArgs& A, const SkDims& d) {
  return CNT ? -log((double)d.m + (double)d.n) : A.norm;
}
template <bool CNT>
__device__ __forceinline__ double sk_log_mu_bin(const SkArgs& A, const SkDims& d) {
  return CNT ? log((double)d.n) + sk_norm<true>(A, d) : A.log_mu_bin;
}
template <bool CNT>
__device__ __forceinline__ double sk_log_nu_bin(const SkArgs& A, const SkDims& d) {
  return CNT ? log((double)d.m) + sk_norm<true>(A, d) : A.log_nu_bin;
}

// exp of a non-positive argument for a sum: v_exp_f32 on x * log2(e).  The product's rounding
// makes the relative error |x| * 2^-24, so the absolute error is at most max(x e^-x) * 2^-24 =
// 2e-8 plus the instruction's own ulp: what an accurately rounded expf gives a sum of such terms,
// at a tenth of the instructions (the pass is otherwise VALU-bound, not bandwidth-bound).
__device__ __forceinline__ void lse_add(double& mx, double& s, double x) {
  const double d = x - mx;
  const double e = (double)__expf(-fabsf((float)d));
  if (d > 0.0) {
    s = fma(s, e, 1.0);
    mx = x;
  } else {
    s += e;
  }
}
__device__ __forceinline__ void lse_merge(double& m1, double& s1, double m2, double s2) {
  const double M = fmax(m1, m2);
  if (M == -INFINITY) return;   // both empty
  s1 = s1 * exp(m1 - M) + s2 * exp(m2 - M);
  m1 = M;
}
__device__ __forceinline__ double sk_alpha(const SkArgs& A) {
  return (double)(A.alpha_p != nullptr ? *A.alpha_p : A.alpha_v);
}

__global__ __launch_bounds__(256) void sk_init_kernel(SkArgs A) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i <= A.m) A.u[(int64_t)b * (A.m + 1) + i] = 0.0;
  if (i <= A.n) A.v[(int64_t)b * A.v_bs + i] = 0.0;
}

template <bool CNT>
__global__ __launch_bounds__(256) void sk_row_kernel(SkArgs A) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const SkDims D = sk_dims<CNT>(A, b);
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), m = D.m, n = D.n;
  if (D.empty || i > m) return;
  const double a = sk_alpha(A);
  const double* v = A.v + (int64_t)b * A.v_bs;
  double mx = -INFINITY, s = 0.0;
  if (i < m) {
    const float* row = A.S + (int64_t)b * A.s_bs + (int64_t)i * A.ld;
    if ((A.ld & 3) == 0 && (A.s_bs & 3) == 0 && (reinterpret_cast<uintptr_t>(A.S) & 15) == 0) {
#pragma unroll 2
      for (int j = lane * 4; j < n; j += 256) {   // v is padded past n + 1
        const float4 x = *reinterpret_cast<const float4*>(row + j);
        const double2 y0 = *reinterpret_cast<const double2*>(v + j);
        const double2 y1 = *reinterpret_cast<const double2*>(v + j + 2);
        lse_add(mx, s, (double)x.x + y0.x);
        if (j + 1 < n) lse_add(mx, s, (double)x.y + y0.y);
        if (j + 2 < n) lse_add(mx, s, (double)x.z + y1.x);
        if (j + 3 < n) lse_add(mx, s, (double)x.w + y1.y);
      }
    } else {
#pragma unroll 4
      for (int j = lane; j < n; j += 64) lse_add(mx, s, (double)row[j] + v[j]);
    }
  } else {
#pragma unroll 4
    for (int j = lane; j < n; j += 64) lse_add(mx, s, a + v[j]);
  }
  if (lane == 0) lse_add(mx, s, a + v[n]);   // the dustbin column
  const double M = wave_max_d(mx);
  s = wave_sum_d(mx == -INFINITY ? 0.0 : s * exp(mx - M));
  if (lane == 0)
    A.u[(int64_t)b * (A.m + 1) + i] =
        (i < m ? sk_norm<CNT>(A, D) : sk_log_mu_bin<CNT>(A, D)) - (M + log(s));
}

// grid (ceil((n+1)/64), chunks, B): 64 columns x one row chunk; wave w takes rows r0 + w + 4 k
// CNT: the chunks are those of the batch's m; a chunk past the sample's dustbin row (row m of the
// sample) has no rows and leaves the empty partial (-inf, 0), which lse_merge passes over.
template <bool CNT>
__global__ __launch_bounds__(256) void sk_col_kernel(SkArgs A) {
  __shared__ double red_m[4][64], red_s[4][64];
  const int b = blockIdx.z, c = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const SkDims D = sk_dims<CNT>(A, b);
  if (D.empty) return;   // the whole workgroup
  const int j = blockIdx.x * 64 + lane, m = D.m, n = D.n;
  const int r0 = c * A.rows, r1 = min(r0 + A.rows, m + 1);
  const double a = sk_alpha(A);
  const double* u = A.u + (int64_t)b * (A.m + 1);
  const float* Sc = A.S + (int64_t)b * A.s_bs + j;
  double mx = -INFINITY, s = 0.0;
  if (j <= n) {
    for (int i = r0 + w; i < r1; i += 16) {
      double x[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ii = i + 4 * q;
        x[q] = (ii < m && j < n) ? (double)Sc[(int64_t)ii * A.ld] : a;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int ii = i + 4 * q;
        if (ii < r1) lse_add(mx, s, x[q] + u[ii]);
      }
    }
  }
  red_m[w][lane] = mx;
  red_s[w][lane] = s;
  __syncthreads();
  if (w != 0 || j > n) return;
#pragma unroll
  for (int q = 1; q < 4; ++q) lse_merge(mx, s, red_m[q][lane], red_s[q][lane]);
  if (A.chunks == 1)
    A.v[(int64_t)b * A.v_bs + j] =
        (j < n ? sk_norm<CNT>(A, D) : sk_log_nu_bin<CNT>(A, D)) - (mx + log(s));
  else
    A.part[((int64_t)b * A.chunks + c) * (A.n + 1) + j] = make_double2(mx, s);
}

template <bool CNT>
__global__ __launch_bounds__(256) void sk_colmerge_kernel(SkArgs A) {
  const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  const SkDims D = sk_dims<CNT>(A, b);
  const int n = D.n;
  if (D.empty || j > n) return;
  const double2* p = A.part + (int64_t)b * A.chunks * (A.n + 1) + j;
  double mx = -INFINITY, s = 0.0;
  for (int c = 0; c < A.chunks; ++c) {
    const double2 q = p[(int64_t)c * (A.n + 1)];
    lse_merge(mx, s, q.x, q.y);
  }
  A.v[(int64_t)b * A.v_bs + j] =
      (j < n ? sk_norm<CNT>(A, D) : sk_log_nu_bin<CNT>(A, D)) - (mx + log(s));
}

// Z + u + v - norm in the reference's order (float64, rounded to fp32 once), written to `out`
// ([B][m+1][n+1]) when asked for, and the row winners over Z[:m, :n] (lowest index on ties).  A
// wave per row.
struct SkBest {
  float val;
  int idx;
};
// CNT: sample b's (m+1) x (n+1) matrix is the top-left block of its padded slot in `out` (dustbin
// row at the sample's m, dustbin column at its n); nothing outside the block is written.
template <bool CNT>
__global__ __launch_bounds__(256) void sk_finish_row_kernel(SkArgs A, float* out, float* rowmax,
                                                            int* rowidx) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const SkDims D = sk_dims<CNT>(A, b);
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), m = D.m, n = D.n;
  if (D.empty || i > m || (out == nullptr && i == m)) return;
  const double a = sk_alpha(A), ui = A.u[(int64_t)b * (A.m + 1) + i];
  const double norm = sk_norm<CNT>(A, D);
  const double* v = A.v + (int64_t)b * A.v_bs;
  const float* row = A.S + (int64_t)b * A.s_bs + (int64_t)i * A.ld;
  float* o = out != nullptr ? out + ((int64_t)b * (A.m + 1) + i) * (A.n + 1) : nullptr;
  float best = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll 4
  for (int j = lane; j <= n; j += 64) {
    const bool inner = i < m && j < n;
    const float z = (float)((((inner ? (double)row[j] : a) + ui) + v[j]) - norm);
    if (o != nullptr) o[j] = z;
    if (inner && z > best) {
      best = z;
      bi = j;
    }
  }
  if (rowmax == nullptr || i >= m) return;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float ov = __shfl_xor(best, d, 64);
    const int oi = __shfl_xor(bi, d, 64);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    rowmax[(int64_t)b * A.m + i] = best;
    rowidx[(int64_t)b * A.m + i] = bi == 0x7fffffff ? 0 : bi;
  }
}

// Column winners over Z[:m, :n] per row chunk (grid (ceil(n/64), chunks, B)), lowest row on ties.
template <bool CNT>
__global__ __launch_bounds__(256) void sk_finish_col_kernel(SkArgs A, SkBest* cpart) {
  __shared__ float red_v[4][64];
  __shared__ int red_i[4][64];
  const int b = blockIdx.z, c = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const SkDims D = sk_dims<CNT>(A, b);
  if (D.empty) return;   // the whole workgroup
  const int j = blockIdx.x * 64 + lane, m = D.m, n = D.n;
  const int r0 = c * A.rows, r1 = min(r0 + A.rows, m);
  const double* u = A.u + (int64_t)b * (A.m + 1);
  const double norm = sk_norm<CNT>(A, D);
  float best = -INFINITY;
  int bi = 0x7fffffff;
  if (j < n) {
    const float* Sc = A.S + (int64_t)b * A.s_bs + j;
    const double vj = A.v[(int64_t)b * A.v_bs + j];
#pragma unroll 4
    for (int i = r0 + w; i < r1; i += 4) {
      const float z = (float)((((double)Sc[(int64_t)i * A.ld] + u[i]) + vj) - norm);
      if (z > best) {
        best = z;
        bi = i;
      }
    }
  }
  red_v[w][lane] = best;
  red_i[w][lane] = bi;
  __syncthreads();
  if (w != 0 || j >= n) return;
#pragma unroll
  for (int q = 1; q < 4; ++q) {
    const float ov = red_v[q][lane];
    const int oi = red_i[q][lane];
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  cpart[((int64_t)b * A.chunks + c) * A.n + j] = SkBest{best, bi};
}

// Mutual check and threshold (superglue.py:310-320).  One workgroup per sample.  CNT (mm, nn: the
// batch's m and n, the strides): entries past the sample's counts, and every entry of a sample
// with an empty side (the reference's empty branch for that pair), are -1 and 0.
template <bool CNT>
__global__ __launch_bounds__(1024) void sg_mutual_kernel(const float* rowmax, const int* rowidx,
                                                         const SkBest* cpart, int chunks, int mm,
                                                         int nn, float thr, int* colidx,
                                                         int64_t* matches0, int64_t* matches1,
                                                         float* mscores0, float* mscores1,
                                                         const int* counts_m, const int* counts_n) {
  const int b = blockIdx.x;
  rowmax += (int64_t)b * mm;
  rowidx += (int64_t)b * mm;
  cpart += (int64_t)b * chunks * nn;
  colidx += (int64_t)b * nn;
  matches0 += (int64_t)b * mm;
  mscores0 += (int64_t)b * mm;
  matches1 += (int64_t)b * nn;
  mscores1 += (int64_t)b * nn;
  int m = mm, n = nn;
  if (CNT) {
    m = sg_count(counts_m, b, mm);
    n = sg_count(counts_n, b, nn);
    if (m == 0 || n == 0) m = n = 0;
    for (int i = m + threadIdx.x; i < mm; i += 1024) {
      matches0[i] = (int64_t)-1;
      mscores0[i] = 0.f;
    }
    for (int j = n + threadIdx.x; j < nn; j += 1024) {
      matches1[j] = (int64_t)-1;
      mscores1[j] = 0.f;
    }
  }
  for (int j = threadIdx.x; j < n; j += 1024) {
    float best = -INFINITY;
    int bi = 0;
    for (int c = 0; c < chunks; ++c) {   // ascending rows: a later chunk wins only if larger
      const SkBest q = cpart[(int64_t)c * nn + j];
      if (q.val > best) {
        best = q.val;
        bi = q.idx;
      }
    }
    colidx[j] = bi;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < m; i += 1024) {
    const int j = rowidx[i];
    const bool mutual = colidx[j] == i;
    const float sc = mutual ? expf(rowmax[i]) : 0.f;
    mscores0[i] = sc;
    matches0[i] = (mutual && sc > thr) ? (int64_t)j : (int64_t)-1;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n; j += 1024) {
    const int i = colidx[j];
    const bool mutual = rowidx[i] == j;
    mscores1[j] = mutual ? mscores0[i] : 0.f;
    matches1[j] = (mutual && matches0[i] != (int64_t)-1) ? (int64_t)i : (int64_t)-1;
  }
}

int sk_chunks(int rows) { return rows <= 2 * kSkRows ? 1 : ceil_div(rows, kSkRows); }

// u, v for `iters` iterations (A.S / ld / m / n / alpha / u / v / part set by the caller).
// CNT: the same launches over the batch's m and n (A.counts_m / A.counts_n say where each sample
// ends; the three constants below are then computed per sample on the device).
template <bool CNT>
int sinkhorn_run(SkArgs& A, int batch, int iters, hipStream_t st) {
  const int m = A.m, n = A.n;
  // norm = -log(m + n), log_mu = [norm] * m + [log(n) + norm], log_nu likewise (:203-205)
  A.norm = -std::log((double)m + (double)n);
  A.log_mu_bin = std::log((double)n) + A.norm;
  A.log_nu_bin = std::log((double)m) + A.norm;
  A.chunks = sk_chunks(m + 1);
  A.rows = A.chunks == 1 ? m + 1 : kSkRows;
  const int mx = m > n ? m : n;
  OP_LAUNCH(K_SG_SINKHORN, st, sk_init_kernel, dim3(ceil_div(mx + 1, 256), batch), dim3(256), 0, st, A);
  // (one chunk: its rows are strided by the waves of a single workgroup per 64 columns)
  const dim3 gcol(ceil_div(n + 1, 64), A.chunks, batch);
  for (int it = 0; it < iters; ++it) {
    OP_LAUNCH(K_SG_SINKHORN, st, sk_row_kernel<CNT>, dim3(ceil_div(m + 1, 4), batch), dim3(256), 0,
              st, A);
    OP_LAUNCH(K_SG_SINKHORN, st, sk_col_kernel<CNT>, gcol, dim3(256), 0, st, A);
    if (A.chunks > 1)
      OP_LAUNCH(K_SG_SINKHORN, st, sk_colmerge_kernel<CNT>, dim3(ceil_div(n + 1, 256), batch),
                dim3(256), 0, st, A);
  }
  return ONEPOSE_OK;
}

size_t v_stride(int n) { return align_up((size_t)n + 1 + 4, 64); }

struct SkPlan {
  double *u, *v;
  double2* part;
  size_t bytes;
};
SkPlan sk_plan(void* ws, int batch, int m, int n) {
  Carve c(ws);
  SkPlan p;
  p.u = c.take<double>((size_t)batch * ((size_t)m + 1));
  p.v = c.take<double>((size_t)batch * v_stride(n));
  p.part = c.take<double2>((size_t)batch * sk_chunks(m + 1) * ((size_t)n + 1));
  p.bytes = align_up(c.off, 256);
  return p;
}

// ------------------------------------------------------------------------------------
// forward plan
// ------------------------------------------------------------------------------------
struct SgPlan {
  float* x[2][2];   // [buffer][side]
  float* qkv[2];
  float* msg[2];
  float* y1[2];
  float *S, *rowstat, *colstat;
  double *u, *v;
  double2* part;
  float* rowmax;
  int* rowidx;
  SkBest* cpart;
  int* colidx;
  int ldS;
  size_t bytes;
};
constexpr int kSgScoreTile = TILE_128x64W8;
// the forward's GEMMs name kernels gemm.hip has (gemm.h kGemmVariants): fp32, register-staged
static_assert(gemm_has_variant(EPI_SCORE, PRO_PLAIN, kSgScoreTile, PM_F32, false, 0) &&
                  gemm_has_variant(EPI_BIAS, PRO_PLAIN, TILE_64x64, PM_F32, false, 0) &&
                  gemm_has_variant(EPI_RESID, PRO_NORM_RELU, TILE_64x64, PM_F32, false, 0),
              "SuperGlue's GEMM tiles");

SgPlan sg_plan(void* ws, int batch, int n0, int n1) {
  Carve c(ws);
  SgPlan p;
  const size_t B = (size_t)batch, n[2] = {(size_t)n0, (size_t)n1};
  for (int s = 0; s < 2; ++s) {
    p.x[0][s] = c.take<float>(B * n[s] * 256);
    p.x[1][s] = c.take<float>(B * n[s] * 256);
    p.qkv[s] = c.take<float>(B * n[s] * 768);
    p.msg[s] = c.take<float>(B * n[s] * 256);
    p.y1[s] = c.take<float>(B * n[s] * 512);
  }
  p.ldS = (n1 + 3) & ~3;
  p.S = c.take<float>(B * n[0] * (size_t)p.ldS);
  const size_t mt = (size_t)ceil_div(n0, gemm_tile_bm(kSgScoreTile)),
               nt = (size_t)ceil_div(n1, gemm_tile_bn(kSgScoreTile));
  p.rowstat = c.take<float>(B * n[0] * nt * 2);
  p.colstat = c.take<float>(B * mt * n[1] * 2);
  p.u = c.take<double>(B * (n[0] + 1));
  p.v = c.take<double>(B * v_stride(n1));
  const size_t ch = (size_t)sk_chunks(n0 + 1);
  p.part = c.take<double2>(B * ch * (n[1] + 1));
  p.rowmax = c.take<float>(B * n[0]);
  p.rowidx = c.take<int>(B * n[0]);
  p.cpart = c.take<SkBest>(B * ch * n[1]);
  p.colidx = c.take<int>(B * n[1]);
  p.bytes = align_up(c.off, 256);
  return p;
}

const char* check_shape(int batch, int n0, int n1) {
  if (batch < 1 || batch > 65535) return "batch must be in [1, 65535]";
  if (n0 < 1 || n1 < 1) return "n0 and n1 must be at least 1 (the caller handles the empty branch)";
  if (n0 > kSgMaxPoints || n1 > kSgMaxPoints) return "at most 16384 points per image";
  return nullptr;
}

}  // namespace
}  // namespace onepose

using namespace onepose;

extern "C" {

int onepose_superglue_version(void) { return 1; }

int onepose_superglue_num_tensors(void) { return (int)sg_specs().size(); }
const char* onepose_superglue_tensor_name(int i) {
  const auto& s = sg_specs();
  return (i >= 0 && i < (int)s.size()) ? s[i].name.c_str() : nullptr;
}
int64_t onepose_superglue_tensor_numel(int i) {
  const auto& s = sg_specs();
  return (i >= 0 && i < (int)s.size()) ? s[i].numel : -1;
}
size_t onepose_superglue_packed_bytes(void) { return (size_t)kSgFloats * 4; }

int onepose_superglue_pack(const float* const* tensors, int n_tensors, void* packed_host) {
  clear_error();
  OP_REQUIRE(tensors != nullptr && packed_host != nullptr, "superglue_pack: null argument");
  OP_REQUIRE(n_tensors == (int)sg_specs().size(), "superglue_pack: %d tensors, expected %d",
             n_tensors, (int)sg_specs().size());
  for (int i = 0; i < n_tensors; ++i)
    OP_REQUIRE(tensors[i] != nullptr, "superglue_pack: tensor %d (%s) is null", i,
               sg_specs()[i].name.c_str());
  float* out = static_cast<float*>(packed_host);
  memset(out, 0, (size_t)kSgFloats * 4);
  int ti = 0;
  const float* bin = tensors[ti++];
  // eval BatchNorm after a conv: y = s (W x + b - mean) + beta, s = gamma / sqrt(var + eps)
  auto bn_scale = [](const float* const* bn, int o) {
    return (double)bn[0][o] / std::sqrt((double)bn[3][o] + kBnEps);
  };
  auto bn_bias = [](const float* const* bn, int o, double s, double b) {
    return s * (b - (double)bn[2][o]) + (double)bn[1][o];
  };
  // keypoint encoder
  const int64_t woff[5] = {kKeW1, kKeW2, kKeW3, kKeW4, kKeW5};
  const int64_t boff[5] = {kKeB1, kKeB2, kKeB3, kKeB4, kKeB5};
  for (int l = 0; l < 5; ++l) {
    const int ci = kEncCh[l], co = kEncCh[l + 1];
    const float *W = tensors[ti], *b = tensors[ti + 1];
    const float* const* bn = l < 4 ? tensors + ti + 2 : nullptr;
    ti += l < 4 ? 6 : 2;
    for (int o = 0; o < co; ++o) {
      const double s = bn ? bn_scale(bn, o) : 1.0;
      for (int c = 0; c < ci; ++c) {
        const float v = (float)(s * (double)W[(int64_t)o * ci + c]);
        if (l < 3) out[woff[l] + (int64_t)c * co + o] = v;   // in-major
        else out[woff[l] + (int64_t)o * ci + c] = v;         // out-major
      }
      out[boff[l] + o] = (float)(bn ? bn_bias(bn, o, s, (double)b[o]) : (double)b[o]);
    }
  }
  for (int i = 0; i < 512; ++i) out[kKeOnes + i] = 1.f;
  // attention layers
  std::vector<double> C((size_t)512 * 256), cb(512);
  for (int l = 0; l < kSgLayers; ++l) {
    float* L = out + kSgLayer0 + (int64_t)l * kLyFloats;
    const float *Wm = tensors[ti], *bm = tensors[ti + 1];
    for (int j = 0; j < 3; ++j) {
      const float *W = tensors[ti + 2 + 2 * j], *b = tensors[ti + 3 + 2 * j];
      for (int h = 0; h < 4; ++h)
        for (int d = 0; d < 64; ++d) {
          const int pr = j * 256 + h * 64 + d, rr = d * 4 + h;
          memcpy(L + kLyWqkv + (int64_t)pr * 256, W + (int64_t)rr * 256, 256 * 4);
          L[kLyBqkv + pr] = b[rr];
        }
    }
    const float *W1 = tensors[ti + 8], *b1 = tensors[ti + 9];
    const float* const* bn = tensors + ti + 10;
    const float *W2 = tensors[ti + 14], *b2 = tensors[ti + 15];
    ti += 16;
    // C = W1[:, 256:] @ Wm (float64), cb = W1[:, 256:] @ bm
    for (int o = 0; o < 512; ++o) {
      const float* w1b = W1 + (int64_t)o * 512 + 256;
      double* Co = C.data() + (size_t)o * 256;
      for (int c = 0; c < 256; ++c) Co[c] = 0.0;
      double acc = 0.0;
      for (int k = 0; k < 256; ++k) {
        const double wk = (double)w1b[k];
        const float* wm = Wm + (int64_t)k * 256;
        for (int c = 0; c < 256; ++c) Co[c] += wk * (double)wm[c];
        acc += wk * (double)bm[k];
      }
      cb[o] = acc;
    }
    for (int o = 0; o < 512; ++o) {
      const double s = bn_scale(bn, o);
      float* row = L + kLyW1 + (int64_t)o * 512;
      for (int c = 0; c < 256; ++c) row[c] = (float)(s * (double)W1[(int64_t)o * 512 + c]);
      for (int h = 0; h < 4; ++h)   // message columns head-major: packed h*64+d <- d*4+h
        for (int d = 0; d < 64; ++d)
          row[256 + h * 64 + d] = (float)(s * C[(size_t)o * 256 + d * 4 + h]);
      L[kLyB1 + o] = (float)bn_bias(bn, o, s, (double)b1[o] + cb[o]);
    }
    memcpy(L + kLyW2, W2, (size_t)256 * 512 * 4);
    memcpy(L + kLyB2, b2, 256 * 4);
  }
  memcpy(out + kSgFinal, tensors[ti], 65536 * 4);
  memcpy(out + kSgFinal + 65536, tensors[ti + 1], 256 * 4);
  out[kSgBin] = bin[0];
  return ONEPOSE_OK;
}

size_t onepose_superglue_workspace_bytes(int batch, int n0, int n1) {
  if (check_shape(batch, n0, n1) != nullptr) return 0;
  return sg_plan(nullptr, batch, n0, n1).bytes;
}

size_t onepose_log_optimal_transport_workspace_bytes(int batch, int m, int n) {
  if (check_shape(batch, m, n) != nullptr) return 0;
  return sk_plan(nullptr, batch, m, n).bytes;
}

}  // extern "C"

// The bodies of the entry points that exist with and without counts: CNT = false is the uniform
// entry (null count / size arrays, the CNT = false kernels), CNT = true the counts entry.
namespace onepose {
namespace {

template <bool CNT>
int lot_entry(const float* scores, int64_t scores_bstride, int batch, int m, int n,
              const int* counts_m, const int* counts_n, float alpha, int iters, float* out,
              void* workspace, size_t workspace_bytes, void* stream) {
  clear_error();
  const char* bad = check_shape(batch, m, n);
  OP_REQUIRE(bad == nullptr, "log_optimal_transport: %s", bad);
  OP_REQUIRE(scores != nullptr && out != nullptr, "log_optimal_transport: null scores / out");
  OP_REQUIRE(iters >= 0, "log_optimal_transport: iters = %d is negative", iters);
  OP_REQUIRE(scores_bstride >= 0, "log_optimal_transport: negative batch stride");
  OP_REQUIRE(workspace != nullptr, "log_optimal_transport: null workspace");
  const SkPlan p = sk_plan(workspace, batch, m, n);
  if (workspace_bytes < p.bytes) {
    set_error("log_optimal_transport: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
    return ONEPOSE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  SkArgs A{};
  A.S = scores;
  A.s_bs = scores_bstride;
  A.ld = n;
  A.m = m;
  A.n = n;
  A.alpha_p = nullptr;
  A.alpha_v = alpha;
  A.u = p.u;
  A.v = p.v;
  A.v_bs = (int64_t)v_stride(n);
  A.part = p.part;
  A.counts_m = counts_m;
  A.counts_n = counts_n;
  int rc;
  if ((rc = sinkhorn_run<CNT>(A, batch, iters, st)) != ONEPOSE_OK) return rc;
  OP_LAUNCH(K_SG_SINKHORN, st, sk_finish_row_kernel<CNT>, dim3(ceil_div(m + 1, 4), batch), dim3(256),
            0, st, A, out, static_cast<float*>(nullptr), static_cast<int*>(nullptr));
  return ONEPOSE_OK;
}

template <bool CNT>
int mha_entry(const float* q, int64_t q_bstride, const float* k, int64_t k_bstride, const float* v,
              int64_t v_bstride, int batch, int n, int m, const int* counts_q, const int* counts_k,
              float* out, int64_t out_bstride, void* stream) {
  clear_error();
  const char* bad = check_shape(batch, n, m);
  OP_REQUIRE(bad == nullptr, "mha_softmax: %s", bad);
  OP_REQUIRE(q != nullptr && k != nullptr && v != nullptr && out != nullptr,
             "mha_softmax: null argument");
  OP_REQUIRE(q_bstride >= 0 && k_bstride >= 0 && v_bstride >= 0 && out_bstride >= 0 &&
                 (q_bstride | k_bstride | v_bstride | out_bstride) % 4 == 0,
             "mha_softmax: batch strides must be non-negative multiples of 4 elements");
  OP_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) |
               reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
             "mha_softmax: pointers must be 16-byte aligned");
  OP_REQUIRE(batch == 1 || out_bstride >= (int64_t)n * 256, "mha_softmax: outputs overlap");
  AttnArgs a{};
  a.batch = batch;
  a.p[0] = AttnProb{q, k, v, out, q_bstride, k_bstride, v_bstride, out_bstride,
                    256, 256, 256, 256, n, m, 0, counts_q, counts_k};
  return attn_launch<CNT>(a, 1, static_cast<hipStream_t>(stream));
}

template <bool CNT>
int sg_forward(const void* packed_weights,
               const float* desc0, int64_t desc0_bstride,
               const float* kpts0, int64_t kpts0_bstride,
               const float* scores0, int64_t scores0_bstride,
               const float* desc1, int64_t desc1_bstride,
               const float* kpts1, int64_t kpts1_bstride,
               const float* scores1, int64_t scores1_bstride,
               int batch, int n0, int n1, int h0, int w0, int h1, int w1,
               const int* counts0, const int* counts1, const int* hw0, const int* hw1,
               int sinkhorn_iters, float match_threshold, int precision,
               int64_t* matches0, int64_t* matches1, float* mscores0,
               float* mscores1, float* log_assignment, void* workspace,
               size_t workspace_bytes, void* stream) {
  clear_error();
  if (precision != ONEPOSE_PREC_FP32) {
    set_error("superglue_match: precision %d: this matcher runs in ONEPOSE_PREC_FP32 only", precision);
    return ONEPOSE_ERR_UNSUPPORTED;
  }
  const char* bad = check_shape(batch, n0, n1);
  OP_REQUIRE(bad == nullptr, "superglue_match: %s", bad);
  OP_REQUIRE(sinkhorn_iters >= 0, "superglue_match: sinkhorn_iters = %d is negative", sinkhorn_iters);
  OP_REQUIRE(h0 > 0 && w0 > 0 && h1 > 0 && w1 > 0, "superglue_match: image sizes must be positive");
  OP_REQUIRE(packed_weights != nullptr && desc0 != nullptr && kpts0 != nullptr &&
                 scores0 != nullptr && desc1 != nullptr && kpts1 != nullptr && scores1 != nullptr,
             "superglue_match: null input");
  OP_REQUIRE(matches0 != nullptr && matches1 != nullptr && mscores0 != nullptr && mscores1 != nullptr,
             "superglue_match: null output");
  OP_REQUIRE(desc0_bstride >= 0 && kpts0_bstride >= 0 && scores0_bstride >= 0 &&
                 desc1_bstride >= 0 && kpts1_bstride >= 0 && scores1_bstride >= 0,
             "superglue_match: negative batch stride");
  if (CNT) {   // a side shared by the batch has one count, the array's n
    OP_REQUIRE(counts0 == nullptr ||
                   (desc0_bstride != 0 && kpts0_bstride != 0 && scores0_bstride != 0),
               "superglue_match: counts0 with image 0 at batch stride 0 (a shared side has no "
               "per-sample counts)");
    OP_REQUIRE(counts1 == nullptr ||
                   (desc1_bstride != 0 && kpts1_bstride != 0 && scores1_bstride != 0),
               "superglue_match: counts1 with image 1 at batch stride 0 (a shared side has no "
               "per-sample counts)");
  }
  OP_REQUIRE(workspace != nullptr, "superglue_match: null workspace");
  OP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0 &&
                 (reinterpret_cast<uintptr_t>(packed_weights) & 15) == 0,
             "superglue_match: workspace must be 256-byte and weights 16-byte aligned");
  const SgPlan p = sg_plan(workspace, batch, n0, n1);
  if (workspace_bytes < p.bytes) {
    set_error("superglue_match: workspace of %zu bytes, %zu needed", workspace_bytes, p.bytes);
    return ONEPOSE_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* wb = static_cast<const float*>(packed_weights);
  const int B = batch, nn[2] = {n0, n1};
  int rc;

  // ---- input stage: descriptors token-major, keypoint encoder, desc + kenc(kpts, scores)
  {
    SgInArgs ia{};
    ia.batch = B;
    const float* in[2][3] = {{desc0, kpts0, scores0}, {desc1, kpts1, scores1}};
    const int64_t bs[2][3] = {{desc0_bstride, kpts0_bstride, scores0_bstride},
                              {desc1_bstride, kpts1_bstride, scores1_bstride}};
    const int hw[2][2] = {{h0, w0}, {h1, w1}};
    const int* cnt[2] = {counts0, counts1};
    const int* hwp[2] = {hw0, hw1};
    for (int s = 0; s < 2; ++s) {
      SgSideIn& P = ia.p[s];
      P.desc = in[s][0];
      P.kpts = in[s][1];
      P.scores = in[s][2];
      P.desc_bs = bs[s][0];
      P.kpts_bs = bs[s][1];
      P.scores_bs = bs[s][2];
      P.n = nn[s];
      const float w = (float)hw[s][1], h = (float)hw[s][0];
      P.cx = w / 2.f;
      P.cy = h / 2.f;
      P.scale = (w > h ? w : h) * 0.7f;
      P.counts = cnt[s];
      P.hw = hwp[s];
      P.xd = p.msg[s];   // free until the first attention
      P.h3 = p.y1[s];    // free until the first MLP
    }
    ia.p[0].tiles = ceil_div(n0, 64) * 4;
    ia.p[1].tiles = ceil_div(n1, 64) * 4;
    OP_LAUNCH(K_SG_INPUT, st, sg_transpose_kernel<CNT>, dim3((ia.p[0].tiles + ia.p[1].tiles) * B),
              dim3(256), 0, st, ia);
    ia.p[0].tiles = ceil_div(n0, kKencTok);
    ia.p[1].tiles = ceil_div(n1, kKencTok);
    OP_LAUNCH(K_SG_INPUT, st, sg_kenc_kernel<CNT>, dim3((ia.p[0].tiles + ia.p[1].tiles) * B), dim3(128),
              0, st, ia, wb);
    GemmArgs a;
    a.nprob = 2;   // layer 4: 128 -> 256 (BatchNorm folded), pre-ReLU, into the QKV buffer
    for (int s = 0; s < 2; ++s)
      a.p[s] = gemm_prob(p.y1[s], 128, wb + kKeW4, 128, wb + kKeB4, p.qkv[s], 256, nn[s], 256, 128, B);
    if ((rc = gemm_launch(EPI_BIAS, PRO_PLAIN, TILE_64x64, a, st, K_SG_INPUT)) != ONEPOSE_OK) return rc;
    for (int s = 0; s < 2; ++s) {   // layer 5 on ReLU(.) + descriptors
      GemmProb& g = a.p[s];
      g = gemm_prob(p.qkv[s], 256, wb + kKeW5, 256, wb + kKeB5, p.x[0][s], 256, nn[s], 256, 256, B);
      g.R = p.msg[s];
      g.ldr = 256;
      g.r_bs = (int64_t)nn[s] * 256;
      g.pro_mean = wb + kKeZeros;
      g.pro_rstd = wb + kKeOnes;
      g.pro_bs = 0;
    }
    if ((rc = gemm_launch(EPI_RESID, PRO_NORM_RELU, TILE_64x64, a, st, K_SG_INPUT)) != ONEPOSE_OK)
      return rc;
  }

  // ---- 18 attention layers
  int cur = 0;
  for (int l = 0; l < kSgLayers; ++l) {
    const float* L = wb + kSgLayer0 + (int64_t)l * kLyFloats;
    const bool cross = (l & 1) != 0;
    GemmArgs a;
    a.nprob = 2;
    for (int s = 0; s < 2; ++s)
      a.p[s] = gemm_prob(p.x[cur][s], 256, L + kLyWqkv, 256, L + kLyBqkv, p.qkv[s], 768, nn[s], 768,
                         256, B);
    if ((rc = gemm_launch(EPI_BIAS, PRO_PLAIN, TILE_64x64, a, st, K_QKV_GEMM)) != ONEPOSE_OK) return rc;
    AttnArgs at{};
    at.batch = B;
    for (int s = 0; s < 2; ++s) {
      const int src = cross ? 1 - s : s;
      at.p[s] = AttnProb{p.qkv[s], p.qkv[src] + 256, p.qkv[src] + 512, p.msg[s],
                         (int64_t)nn[s] * 768, (int64_t)nn[src] * 768, (int64_t)nn[src] * 768,
                         (int64_t)nn[s] * 256, 768, 768, 768, 256, nn[s], nn[src], 0,
                         s == 0 ? counts0 : counts1, src == 0 ? counts0 : counts1};
    }
    if ((rc = attn_launch<CNT>(at, 2, st)) != ONEPOSE_OK) return rc;
    for (int s = 0; s < 2; ++s) {   // MLP conv 1 on cat[x, message]
      GemmProb& g = a.p[s];
      g = gemm_prob(p.x[cur][s], 256, L + kLyW1, 512, L + kLyB1, p.y1[s], 512, nn[s], 512, 512, B);
      g.ksplit = 256;
      g.A1 = p.msg[s];
      g.lda1 = 256;
      g.a1_bs = (int64_t)nn[s] * 256;
    }
    if ((rc = gemm_launch(EPI_BIAS, PRO_PLAIN, TILE_64x64, a, st, K_MLP1)) != ONEPOSE_OK) return rc;
    for (int s = 0; s < 2; ++s) {   // MLP conv 2 on ReLU(.) + residual
      GemmProb& g = a.p[s];
      g = gemm_prob(p.y1[s], 512, L + kLyW2, 512, L + kLyB2, p.x[cur ^ 1][s], 256, nn[s], 256, 512, B);
      g.R = p.x[cur][s];
      g.ldr = 256;
      g.r_bs = (int64_t)nn[s] * 256;
      g.pro_mean = wb + kKeZeros;
      g.pro_rstd = wb + kKeOnes;
      g.pro_bs = 0;
    }
    if ((rc = gemm_launch(EPI_RESID, PRO_NORM_RELU, TILE_64x64, a, st, K_MLP2)) != ONEPOSE_OK)
      return rc;
    cur ^= 1;
  }

  // ---- final projection and scores / 16 (descriptor_dim ** .5)
  {
    GemmArgs a;
    a.nprob = 2;
    for (int s = 0; s < 2; ++s)
      a.p[s] = gemm_prob(p.x[cur][s], 256, wb + kSgFinal, 256, wb + kSgFinal + 65536, p.msg[s], 256,
                         nn[s], 256, 256, B);
    if ((rc = gemm_launch(EPI_BIAS, PRO_PLAIN, TILE_64x64, a, st, K_FINAL)) != ONEPOSE_OK) return rc;
    a.nprob = 1;
    a.p[0] = gemm_prob(p.msg[0], 256, p.msg[1], 256, nullptr, p.S, p.ldS, n0, n1, 256, B);
    a.p[0].w_bs = (int64_t)n1 * 256;
    a.p[0].scale = 16.f;
    a.p[0].rowstat = p.rowstat;
    a.p[0].colstat = p.colstat;
    if ((rc = gemm_launch(EPI_SCORE, PRO_PLAIN, kSgScoreTile, a, st, K_SCORE)) != ONEPOSE_OK) return rc;
  }

  // ---- optimal transport and matches
  SkArgs A{};
  A.S = p.S;
  A.s_bs = (int64_t)n0 * p.ldS;
  A.ld = p.ldS;
  A.m = n0;
  A.n = n1;
  A.alpha_p = wb + kSgBin;
  A.u = p.u;
  A.v = p.v;
  A.v_bs = (int64_t)v_stride(n1);
  A.part = p.part;
  A.counts_m = counts0;
  A.counts_n = counts1;
  if ((rc = sinkhorn_run<CNT>(A, B, sinkhorn_iters, st)) != ONEPOSE_OK) return rc;
  OP_LAUNCH(K_SG_SINKHORN, st, sk_finish_row_kernel<CNT>, dim3(ceil_div(n0 + 1, 4), B), dim3(256), 0,
            st, A, log_assignment, p.rowmax, p.rowidx);
  OP_LAUNCH(K_SG_MATCH, st, sk_finish_col_kernel<CNT>, dim3(ceil_div(n1, 64), A.chunks, B), dim3(256),
            0, st, A, p.cpart);
  OP_LAUNCH(K_SG_MATCH, st, sg_mutual_kernel<CNT>, dim3(B), dim3(1024), 0, st, p.rowmax, p.rowidx,
            p.cpart, A.chunks, n0, n1, match_threshold, p.colidx, matches0, matches1, mscores0,
            mscores1, counts0, counts1);
  return ONEPOSE_OK;
}

}  // namespace
}  // namespace onepose

extern "C" {

int onepose_superglue_counts_version(void) { return 1; }

int onepose_log_optimal_transport(const float* scores, int64_t scores_bstride, int batch, int m,
                                  int n, float alpha, int iters, float* out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  return lot_entry<false>(scores, scores_bstride, batch, m, n, nullptr, nullptr, alpha, iters, out,
                          workspace, workspace_bytes, stream);
}

int onepose_log_optimal_transport_counts(const float* scores, int64_t scores_bstride, int batch,
                                         int m, int n, const int* counts_m, const int* counts_n,
                                         float alpha, int iters, float* out, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  return lot_entry<true>(scores, scores_bstride, batch, m, n, counts_m, counts_n, alpha, iters, out,
                         workspace, workspace_bytes, stream);
}

int onepose_mha_softmax(const float* q, int64_t q_bstride, const float* k, int64_t k_bstride,
                        const float* v, int64_t v_bstride, int batch, int n, int m, float* out,
                        int64_t out_bstride, void* stream) {
  return mha_entry<false>(q, q_bstride, k, k_bstride, v, v_bstride, batch, n, m, nullptr, nullptr,
                          out, out_bstride, stream);
}

int onepose_mha_softmax_counts(const float* q, int64_t q_bstride, const float* k, int64_t k_bstride,
                               const float* v, int64_t v_bstride, int batch, int n, int m,
                               const int* counts_q, const int* counts_k, float* out,
                               int64_t out_bstride, void* stream) {
  return mha_entry<true>(q, q_bstride, k, k_bstride, v, v_bstride, batch, n, m, counts_q, counts_k,
                         out, out_bstride, stream);
}

int onepose_superglue_match(const void* packed_weights,
                            const float* desc0, int64_t desc0_bstride,
                            const float* kpts0, int64_t kpts0_bstride,
                            const float* scores0, int64_t scores0_bstride,
                            const float* desc1, int64_t desc1_bstride,
                            const float* kpts1, int64_t kpts1_bstride,
                            const float* scores1, int64_t scores1_bstride,
                            int batch, int n0, int n1, int h0, int w0, int h1, int w1,
                            int sinkhorn_iters, float match_threshold, int precision,
                            int64_t* matches0, int64_t* matches1, float* mscores0,
                            float* mscores1, float* log_assignment, void* workspace,
                            size_t workspace_bytes, void* stream) {
  return sg_forward<false>(packed_weights, desc0, desc0_bstride, kpts0, kpts0_bstride, scores0,
                           scores0_bstride, desc1, desc1_bstride, kpts1, kpts1_bstride, scores1,
                           scores1_bstride, batch, n0, n1, h0, w0, h1, w1, nullptr, nullptr, nullptr,
                           nullptr, sinkhorn_iters, match_threshold, precision, matches0, matches1,
                           mscores0, mscores1, log_assignment, workspace, workspace_bytes, stream);
}

int onepose_superglue_match_counts(const void* packed_weights,
                                   const float* desc0, int64_t desc0_bstride,
                                   const float* kpts0, int64_t kpts0_bstride,
                                   const float* scores0, int64_t scores0_bstride,
                                   const float* desc1, int64_t desc1_bstride,
                                   const float* kpts1, int64_t kpts1_bstride,
                                   const float* scores1, int64_t scores1_bstride,
                                   int batch, int n0, int n1, int h0, int w0, int h1, int w1,
                                   const int* counts0, const int* counts1, const int* hw0,
                                   const int* hw1, int sinkhorn_iters, float match_threshold,
                                   int precision, int64_t* matches0, int64_t* matches1,
                                   float* mscores0, float* mscores1, float* log_assignment,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  return sg_forward<true>(packed_weights, desc0, desc0_bstride, kpts0, kpts0_bstride, scores0,
                          scores0_bstride, desc1, desc1_bstride, kpts1, kpts1_bstride, scores1,
                          scores1_bstride, batch, n0, n1, h0, w0, h1, w1, counts0, counts1, hw0, hw1,
                          sinkhorn_iters, match_threshold, precision, matches0, matches1, mscores0,
                          mscores1, log_assignment, workspace, workspace_bytes, stream);
}

}  // extern "C"
