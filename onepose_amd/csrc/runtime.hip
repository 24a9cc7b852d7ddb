// What every translation unit of libonepose_hip shares at run time (declared in common.h): the
// per-thread error string behind onepose_last_error, and the launch-profiling state behind
// OP_LAUNCH's hooks and the onepose_profile_* entry points.  No kernels.
#include <algorithm>
#include <cstdarg>
#include <vector>

#include "common.h"

namespace onepose {

// ------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
}
void clear_error() { g_last_error.clear(); }

// ------------------------------------------------------------------------------------
// launch profiling
// ------------------------------------------------------------------------------------
namespace {
struct Prof {
  uint64_t mask = 0;
  bool device = false;   // device-stamp mode
  std::vector<hipEvent_t> ev;
  std::vector<int> kinds;
  int n = 0;
  StampAcc* acc[K_NUM_KINDS] = {};   // device, kStampPool sites, allocated per stamped kind
  int next[K_NUM_KINDS] = {};   // round-robin pool cursor per kind
};
// Each launch (or graph node captured while stamping) gets its own accumulator from the
// kind's pool, so launches of one kind that run concurrently (several match streams)
// never share one; a graph node keeps its accumulator across replays, which of the same
// graph are serialised.
// Launch sites per kind: a graph node keeps its site; eager launches cycle through the pool,
// and 120 is a multiple of the per-frame launch counts (8 mlp1, 12 SuperPoint convs), so a
// site always sees the same grid (the ticket -> launch arithmetic divides by its wave count).
constexpr int kStampPool = 120;
Prof g_prof;
const char* kKindNames[K_NUM_KINDS] = {
    "transpose_in", "gat", "qkv_gemm", "kv_reduce", "m_fold", "mlp1_gemm",
    "stats_finalize", "mlp2_gemm", "final_gemm", "l2norm", "score_gemm", "softmax_reduce",
    "conf", "mutual", "select", "pnp_ransac", "pnp_refit", "pose_error", "sample_desc",
    "sp_conv", "sp_nms", "sp_select", "sp_desc", "sg_input", "sg_attention", "sg_sinkhorn",
    "sg_match"};
}  // namespace

StampAcc* prof_stamp_slot(int kind) {
  if (!g_prof.device || !((g_prof.mask >> kind) & 1ull) || g_prof.acc[kind] == nullptr)
    return nullptr;
  const int i = g_prof.next[kind]++ % kStampPool;
  return g_prof.acc[kind] + i;
}

void prof_pre(int kind, hipStream_t s) {
  if (g_prof.device) return;
  if (!((g_prof.mask >> kind) & 1ull) || 2 * g_prof.n + 1 >= (int)g_prof.ev.size()) return;
  (void)hipEventRecord(g_prof.ev[2 * g_prof.n], s);
}
void prof_post(int kind, hipStream_t s) {
  if (g_prof.device) return;
  if (!((g_prof.mask >> kind) & 1ull) || 2 * g_prof.n + 1 >= (int)g_prof.ev.size()) return;
  (void)hipEventRecord(g_prof.ev[2 * g_prof.n + 1], s);
  g_prof.kinds[g_prof.n] = kind;
  ++g_prof.n;
}

}  // namespace onepose

using namespace onepose;

extern "C" {

const char* onepose_last_error(void) { return g_last_error.c_str(); }
int onepose_abi_version(void) { return 9; }

int onepose_profile_begin(uint64_t kind_mask, int capacity) {
  clear_error();
  OP_REQUIRE(capacity >= 0, "profile: capacity %d", capacity);
  const size_t need = 2 * (size_t)capacity + 2;
  while (g_prof.ev.size() < need) {
    hipEvent_t e;
    OP_HIP(hipEventCreate(&e));
    g_prof.ev.push_back(e);
  }
  g_prof.kinds.assign(capacity + 1, -1);
  g_prof.n = 0;
  g_prof.mask = kind_mask;
  g_prof.device = false;
  return ONEPOSE_OK;
}

int onepose_profile_begin_device(uint64_t kind_mask) {
  clear_error();
  // per stamped kind: allocated once (graph nodes keep their sites' addresses), zeroed on
  // every call (all zero = armed)
  OP_HIP(hipDeviceSynchronize());
  for (int k = 0; k < K_NUM_KINDS; ++k) {
    if (!((kind_mask >> k) & 1ull)) continue;
    if (g_prof.acc[k] == nullptr)
      OP_HIP(hipMalloc(&g_prof.acc[k], sizeof(StampAcc) * kStampPool));
    OP_HIP(hipMemset(g_prof.acc[k], 0, sizeof(StampAcc) * kStampPool));
  }
  OP_HIP(hipDeviceSynchronize());
  g_prof.n = 0;
  g_prof.mask = kind_mask;
  g_prof.device = true;
  return ONEPOSE_OK;
}

int onepose_profile_end_device(int64_t* launches, double* total_ms, int n_kinds) {
  clear_error();
  OP_REQUIRE(g_prof.device, "profile_end_device: device stamping not active");
  g_prof.device = false;
  const uint64_t mask = g_prof.mask;
  g_prof.mask = 0;
  OP_HIP(hipDeviceSynchronize());
  std::vector<unsigned long long> tot(K_NUM_KINDS, 0ull), cnt(K_NUM_KINDS, 0ull);
  std::vector<StampAcc> pool(kStampPool);
  for (int k = 0; k < K_NUM_KINDS; ++k) {
    if (!((mask >> k) & 1ull) || g_prof.acc[k] == nullptr) continue;
    OP_HIP(hipMemcpy(pool.data(), g_prof.acc[k], sizeof(StampAcc) * kStampPool,
                     hipMemcpyDeviceToHost));
    for (const StampAcc& s : pool)   // launches past kStampRecs per site (s.overflow) dropped
      for (int e = 0; e < kStampRecs; ++e) {
        unsigned long long st = ~0ull, en = 0ull;
        for (int j = 0; j < kStampShards; ++j) {
          const StampRec& r = s.rec[e][j];
          if (r.end == 0) continue;
          st = std::min(st, ~r.nstart);
          en = std::max(en, r.end);
        }
        if (en == 0) continue;
        tot[k] += en > st ? en - st : 0ull;
        ++cnt[k];
      }
  }
  int dev = 0, khz = 0;
  OP_HIP(hipGetDevice(&dev));
  OP_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
  OP_REQUIRE(khz > 0, "profile: wall clock rate unavailable");
  for (int k = 0; k < n_kinds; ++k) {
    const bool ok = k < K_NUM_KINDS;
    if (launches) launches[k] = ok ? (int64_t)cnt[k] : 0;
    if (total_ms) total_ms[k] = ok ? (double)tot[k] / khz : 0.0;
  }
  return ONEPOSE_OK;
}

int onepose_profile_end(int* kinds, float* ms, int capacity, int* count) {
  clear_error();
  g_prof.mask = 0;
  const int n = g_prof.n;
  if (count) *count = n;
  if (n > 0) OP_HIP(hipEventSynchronize(g_prof.ev[2 * n - 1]));
  for (int i = 0; i < n && i < capacity; ++i) {
    float t = 0.f;
    OP_HIP(hipEventElapsedTime(&t, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]));
    if (ms) ms[i] = t;
    if (kinds) kinds[i] = g_prof.kinds[i];
  }
  g_prof.n = 0;
  return ONEPOSE_OK;
}

const char* onepose_profile_kind_name(int kind) {
  return (kind >= 0 && kind < K_NUM_KINDS) ? kKindNames[kind] : nullptr;
}

}  // extern "C"
