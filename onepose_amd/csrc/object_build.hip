// The object builder (the reference's postprocess stage, run.py:196-249): SfM point filter,
// greedy merge of close points and the lifting of 2D descriptors onto the merged 3D points.
// The arithmetic contract is stated in include/onepose_hip.h; tests/object_builder_oracle.py
// restates it in numpy and the GPU tests ask for bit-equality, so every floating-point step below
// is a separate operation in the order written (contraction is off for this file).
//
//   ob_filter_kernel        stable compaction by track length and 3D box, one workgroup walking
//                           the points 1024 at a time (a workgroup scan of the keep flags)
//   ob_count_kernel         neighbours of row j within the radius, one wave per row
//   ob_scan_kernel          exclusive scan of the counts, the capacity check, one workgroup
//   ob_fill_kernel          the same walk as the count, lanes placed by a ballot prefix, so a row
//                           comes out ascending without a sort
//   ob_merge_kernel         the greedy pass, one wave: a run of rows that are each their own only
//                           neighbour at once, the other rows one at a time; recorded points are a
//                           bitmap in LDS
//   ob_lift_check_kernel    segment starts, and every index the lifting will read through, checked
//   ob_lift_kernel          one thread per (point, channel): gather, collect, sequential mean
//   ob_leaves_kernel        the leaf gather
// No floating-point atomics, nothing between workgroups, no spin wait.
#include <limits.h>
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace onepose {
namespace {

constexpr int kObMaxPoints = 65536;        // radius_neighbours / merge_greedy
constexpr int kObMaxFilter = 1 << 24;      // filter_points
constexpr int kObMaxDim = 1024;
constexpr int kObMaxObs = 1 << 28;         // observations / leaf columns
constexpr int kObScanThreads = 1024;

__device__ __forceinline__ unsigned long long lanes_below(int lane) {
  return (1ull << lane) - 1ull;
}

// Exclusive prefix of v over the 1024 threads of the workgroup; *total = the sum.  wsum: 16 ints
// of LDS.  Two barriers; safe to call again at once.
__device__ __forceinline__ int block_excl_scan(int v, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kObScanThreads / 64; ++w) {
    const int s = wsum[w];
    if (w < wave) off += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return off + inc - v;
}

// ------------------------------------------------------------------ filter
__global__ __launch_bounds__(kObScanThreads) void ob_filter_kernel(
    const double* __restrict__ xyz, const int* __restrict__ track_len, int n, int min_track,
    const double* __restrict__ corners, float* __restrict__ xyz_out, int* __restrict__ index_out,
    int* __restrict__ count) {
  __shared__ int wsum[kObScanThreads / 64];
  float c4[3] = {0.f, 0.f, 0.f}, v[3][3] = {}, vv[3] = {0.f, 0.f, 0.f};
  if (corners != nullptr) {
    const int other[3] = {5, 0, 7};
    for (int k = 0; k < 3; ++k) c4[k] = (float)corners[4 * 3 + k];
    for (int a = 0; a < 3; ++a) {
      for (int k = 0; k < 3; ++k) v[a][k] = (float)corners[other[a] * 3 + k] - c4[k];
      vv[a] = (v[a][0] * v[a][0] + v[a][1] * v[a][1]) + v[a][2] * v[a][2];
    }
  }
  int base = 0;
  for (int start = 0; start < n; start += kObScanThreads) {
    const int i = start + (int)threadIdx.x;
    bool keep = false;
    float p[3] = {0.f, 0.f, 0.f};
    if (i < n) {
      for (int k = 0; k < 3; ++k) p[k] = (float)xyz[(int64_t)i * 3 + k];
      keep = track_len == nullptr || track_len[i] >= min_track;
      if (keep && corners != nullptr) {
        const float q0 = p[0] - c4[0], q1 = p[1] - c4[1], q2 = p[2] - c4[2];
        for (int a = 0; a < 3; ++a) {
          const float m = (q0 * v[a][0] + q1 * v[a][1]) + q2 * v[a][2];
          keep = keep && (0.f < m) && (m < vv[a]);
        }
      }
    }
    int total;
    const int off = block_excl_scan(keep ? 1 : 0, wsum, &total);   // kept points before this one
    if (keep) {
      const int pos = base + off;   // pos <= i < n
      for (int k = 0; k < 3; ++k) xyz_out[(int64_t)pos * 3 + k] = p[k];
      index_out[pos] = i;
    }
    base += total;
  }
  if (threadIdx.x == 0) count[0] = base;
}

// ------------------------------------------------------------------ radius neighbours
// true iff i is a neighbour of the row whose point is (xj, yj, zj); `bound` is a value no
// neighbour's squared distance exceeds (thr^2 with room), so most waves skip the square root
template <typename T>
__device__ __forceinline__ bool ob_near(const T* __restrict__ xyz, int i, int j, int n, double xj,
                                        double yj, double zj, double thr, double bound) {
  bool cand = false;
  double s = 0.0;
  if (i < n) {
    const double dx = (double)xyz[(int64_t)i * 3 + 0] - xj;
    const double dy = (double)xyz[(int64_t)i * 3 + 1] - yj;
    const double dz = (double)xyz[(int64_t)i * 3 + 2] - zj;
    s = (dx * dx + dy * dy) + dz * dz;
    cand = s <= bound;
  }
  bool hit = false;
  if (__any(cand)) hit = cand && sqrt(s) < thr;
  return hit || (i == j && i < n);
}

template <typename T>
__global__ __launch_bounds__(256) void ob_count_kernel(const T* __restrict__ xyz, int n, double thr,
                                                       double bound, int* __restrict__ row_start) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;
  const double xj = (double)xyz[(int64_t)j * 3], yj = (double)xyz[(int64_t)j * 3 + 1],
               zj = (double)xyz[(int64_t)j * 3 + 2];
  int cnt = 0;
  for (int i0 = 0; i0 < n; i0 += 64)
    cnt += __popcll(__ballot(ob_near(xyz, i0 + lane, j, n, xj, yj, zj, thr, bound)));
  if (lane == 0) row_start[j] = cnt;
}

// row_start [n] counts -> exclusive starts, row_start[n] = total; info[0] = total, info[1] =
// 0 fits, 1 over the capacity, 2 over 2^31 - 1 (the starts are then clamped, and unused)
__global__ __launch_bounds__(kObScanThreads) void ob_scan_kernel(int* __restrict__ row_start, int n,
                                                                 int64_t capacity,
                                                                 int64_t* __restrict__ info) {
  __shared__ int wsum[kObScanThreads / 64];
  int64_t base = 0;
  for (int start = 0; start < n; start += kObScanThreads) {
    const int i = start + (int)threadIdx.x;
    const int c = i < n ? row_start[i] : 0;   // <= 65536 each: a chunk's sum is < 2^27
    int total;
    const int off = block_excl_scan(c, wsum, &total);
    const int64_t s = base + off;
    if (i < n) row_start[i] = s > INT_MAX ? INT_MAX : (int)s;
    base += total;
  }
  if (threadIdx.x == 0) {
    row_start[n] = base > INT_MAX ? INT_MAX : (int)base;
    info[0] = base;
    info[1] = base > INT_MAX ? 2 : base > capacity ? 1 : 0;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ob_fill_kernel(const T* __restrict__ xyz, int n, double thr,
                                                      double bound,
                                                      const int* __restrict__ row_start,
                                                      const int64_t* __restrict__ info,
                                                      int* __restrict__ cols) {
  if (info[1] != 0) return;   // the list does not fit: nothing of it is written
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;
  const double xj = (double)xyz[(int64_t)j * 3], yj = (double)xyz[(int64_t)j * 3 + 1],
               zj = (double)xyz[(int64_t)j * 3 + 2];
  // the count pass found row_start[j + 1] - row_start[j] hits with the same arithmetic, so the
  // positions stay below row_start[n] <= capacity; `end` keeps that true whatever happens
  int pos = row_start[j];
  const int end = row_start[j + 1];
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const bool hit = ob_near(xyz, i, j, n, xj, yj, zj, thr, bound);
    const unsigned long long b = __ballot(hit);
    const int at = pos + __popcll(b & lanes_below(lane));
    if (hit && at < end) cols[at] = i;
    pos += __popcll(b);
  }
}

// ------------------------------------------------------------------ greedy merge
__global__ __launch_bounds__(256) void ob_fill_int_kernel(int* __restrict__ p, int n, int value) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = value;
}

template <typename T>
__global__ __launch_bounds__(64) void ob_merge_kernel(
    const T* __restrict__ xyz, int n, const int* __restrict__ row_start,
    const int* __restrict__ cols, int* __restrict__ cluster_of, int* __restrict__ member_start,
    int* __restrict__ members, double* __restrict__ mean, int* __restrict__ info) {
  __shared__ unsigned int rec[kObMaxPoints / 32];   // one bit per recorded point
  const int lane = threadIdx.x;
  for (int w = lane; w < kObMaxPoints / 32; w += 64) rec[w] = 0u;
  wave_lds_sync();
  const int64_t total = row_start[n];
  int nc = 0, nm = 0;   // clusters and members so far (wave-uniform)
  bool bad = false;
  for (int j0 = 0; j0 < n && !bad; j0 += 64) {
    const int j = j0 + lane;
    int rs = 0, len = 0;
    if (j < n) {
      rs = row_start[j];
      len = row_start[j + 1] - rs;
    }
    const bool in_range = j >= n || (rs >= 0 && len >= 1 && (int64_t)rs + len <= total);
    if (!__all(in_range)) {
      bad = true;
      break;
    }
    // Most rows hold their own point alone, which no earlier cluster can have recorded: a run of
    // such rows becomes a run of clusters at once.  The other rows are taken one at a time.
    const bool alone = j >= n || (len == 1 && cols[rs] == j);
    const int rows = n - j0 < 64 ? n - j0 : 64;
    const unsigned long long multi = __ballot(!alone);   // lanes >= rows are `alone`
    int pos = 0;
    while (pos < rows && !bad) {
      const unsigned long long rest = multi >> pos;
      const int stop = rest != 0ull ? pos + __ffsll(rest) - 1 : rows;   // the next row not alone
      if (stop > pos) {
        const bool in_run = lane >= pos && lane < stop;   // then j < n
        const bool fresh = in_run && ((rec[j >> 5] >> (j & 31)) & 1u) == 0u;
        const unsigned long long b = __ballot(fresh);
        if (nm + __popcll(b) > n) {   // more members than points: not a CSR of this point set
          bad = true;
          break;
        }
        const int k = __popcll(b & lanes_below(lane));
        if (fresh) {   // nc + k <= nm + k < n
          const int c = nc + k;
          cluster_of[j] = c;
          member_start[c] = nm + k;
          members[nm + k] = j;
          for (int a = 0; a < 3; ++a)   // x / 1 is x
            mean[(int64_t)c * 3 + a] = (double)xyz[(int64_t)j * 3 + a];
          atomicOr(&rec[j >> 5], 1u << (j & 31));
        }
        nc += __popcll(b);
        nm += __popcll(b);
        wave_lds_sync();
      }
      pos = stop + 1;
      if (stop >= rows) break;
      const int rs_r = __shfl(rs, stop, 64), len_r = __shfl(len, stop, 64);
      bool seen = false, wild = false;
      for (int k0 = 0; k0 < len_r; k0 += 64) {
        const int k = k0 + lane;
        if (k < len_r) {
          const int i = cols[rs_r + k];
          if ((unsigned)i >= (unsigned)n)
            wild = true;
          else if ((rec[i >> 5] >> (i & 31)) & 1u)
            seen = true;
        }
      }
      if (__any(wild)) {   // not a CSR of this point set
        bad = true;
        break;
      }
      if (__any(seen)) continue;   // skipped: some neighbour already belongs to a cluster
      if (nm + len_r > n) {        // more members than points: a row names a point twice
        bad = true;
        break;
      }
      const int c = nc;
      if (lane == 0) member_start[c] = nm;
      T sx = (T)0, sy = (T)0, sz = (T)0;
      for (int k0 = 0; k0 < len_r; k0 += 64) {
        const int k = k0 + lane;
        T x = (T)0, y = (T)0, z = (T)0;
        if (k < len_r) {
          const int i = cols[rs_r + k];   // checked above
          x = xyz[(int64_t)i * 3];
          y = xyz[(int64_t)i * 3 + 1];
          z = xyz[(int64_t)i * 3 + 2];
          members[nm + k] = i;
          cluster_of[i] = c;
          atomicOr(&rec[i >> 5], 1u << (i & 31));
        }
        const int cnt = len_r - k0 < 64 ? len_r - k0 : 64;
        for (int q = 0; q < cnt; ++q) {   // the row's order, one addition at a time
          const T xq = __shfl(x, q, 64), yq = __shfl(y, q, 64), zq = __shfl(z, q, 64);
          if (k0 == 0 && q == 0) {
            sx = xq;
            sy = yq;
            sz = zq;
          } else {
            sx = sx + xq;
            sy = sy + yq;
            sz = sz + zq;
          }
        }
      }
      if (lane == 0) {
        const T d = (T)len_r;
        mean[(int64_t)c * 3 + 0] = (double)(sx / d);
        mean[(int64_t)c * 3 + 1] = (double)(sy / d);
        mean[(int64_t)c * 3 + 2] = (double)(sz / d);
      }
      nm += len_r;
      nc += 1;
      wave_lds_sync();
    }
  }
  if (lane == 0) {
    if (!bad) member_start[nc] = nm;
    info[0] = bad ? 0 : nc;
    info[1] = bad ? 1 : 0;
  }
}

// ------------------------------------------------------------------ lifting
struct ObLift {
  const float* bank;
  int64_t bank_numel;
  const int64_t* block_offset;
  const int* block_cols;
  int n_blocks;
  const int* obs_block;
  const int* obs_feat;
  int n_obs;
  const int* seg_len;
  int n3, dim;
  int* seg_start;
  double* collected;
  double* mean64;
  float* mean32;
  int* info;
};

// info[0]: 0 ok, 1 a segment shorter than 1 (or longer than n_obs), 2 the segments do not add up
// to n_obs, 3 a block outside the bank, 4 an observation outside its block; info[1]: the
// smallest offending index (for 2, the sum clamped to int)
__global__ __launch_bounds__(kObScanThreads) void ob_lift_check_kernel(ObLift a) {
  __shared__ int wsum[kObScanThreads / 64];
  __shared__ int who;
  const int tid = threadIdx.x;
  if (tid == 0) who = INT_MAX;
  __syncthreads();
  // every thread reads the same offender between two barriers, so `status` stays uniform and
  // the barriers below are met by all or by none
  auto settle = [&]() {
    __syncthreads();
    const int w = who;
    __syncthreads();
    return w;
  };
  for (int p = tid; p < a.n3; p += kObScanThreads) {
    const int k = a.seg_len[p];
    if (k < 1 || k > a.n_obs) atomicMin(&who, p);
  }
  int status = 0, where = settle();
  if (where != INT_MAX) status = 1;
  if (status == 0) {
    int64_t base = 0;
    for (int start = 0; start < a.n3; start += kObScanThreads) {
      const int p = start + tid;
      const int k = p < a.n3 ? a.seg_len[p] : 0;   // chunk sums may wrap only when base is already
      int total;                                   // over n_obs; caught below through base
      const int off = block_excl_scan(k, wsum, &total);
      if (p < a.n3) {
        const int64_t s = base + (unsigned)off;
        a.seg_start[p] = s > INT_MAX ? INT_MAX : (int)s;
      }
      base += (unsigned)total;
      if (base > a.n_obs) break;   // uniform
    }
    if (base != a.n_obs) {
      status = 2;
      where = base > INT_MAX ? INT_MAX : (int)base;
    } else if (tid == 0) {
      a.seg_start[a.n3] = a.n_obs;
    }
  }
  if (status == 0) {
    for (int b = tid; b < a.n_blocks; b += kObScanThreads) {
      const int64_t off = a.block_offset[b];
      const int nc = a.block_cols[b];
      if (off < 0 || nc < 0 || off > a.bank_numel || (int64_t)nc * a.dim > a.bank_numel - off)
        atomicMin(&who, b);
    }
    where = settle();
    if (where != INT_MAX) status = 3;
  }
  if (status == 0) {
    for (int o = tid; o < a.n_obs; o += kObScanThreads) {
      const int b = a.obs_block[o], f = a.obs_feat[o];
      if (b < 0 || b >= a.n_blocks || f < 0 || f >= a.block_cols[b]) atomicMin(&who, o);
    }
    where = settle();
    if (where != INT_MAX) status = 4;
  }
  if (tid == 0) {
    a.info[0] = status;
    a.info[1] = status == 0 ? 0 : where;
  }
}

__global__ __launch_bounds__(256) void ob_lift_kernel(ObLift a) {
  if (a.info[0] != 0) return;   // refused on the device: nothing is written
  const int p = blockIdx.x * 64 + threadIdx.x;
  const int c = blockIdx.y * 4 + threadIdx.y;
  if (p >= a.n3 || c >= a.dim) return;
  const int s0 = a.seg_start[p], k = a.seg_len[p];   // checked: s0 + k <= n_obs, k >= 1
  double s = 0.0;
  for (int o = s0; o < s0 + k; ++o) {
    const int b = a.obs_block[o], f = a.obs_feat[o];   // checked
    const double v = (double)a.bank[a.block_offset[b] + (int64_t)c * a.block_cols[b] + f];
    a.collected[(int64_t)c * a.n_obs + o] = v;
    s = o == s0 ? v : s + v;
  }
  const double m = s / (double)k;
  a.mean64[(int64_t)c * a.n3 + p] = m;
  a.mean32[(int64_t)c * a.n3 + p] = (float)m;
}

__global__ __launch_bounds__(256) void ob_leaves_kernel(const double* __restrict__ collected,
                                                        int n_obs, int dim,
                                                        const int64_t* __restrict__ cols,
                                                        int n_cols, float* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const int c = blockIdx.y * 4 + threadIdx.y;
  if (i >= n_cols || c >= dim) return;
  const int64_t src = cols[i];
  float v;
  if (src == (int64_t)n_obs)
    v = 1.0f;   // the dustbin leaf
  else if (src < 0 || src > (int64_t)n_obs)
    v = __builtin_nanf("");
  else
    v = (float)collected[(int64_t)c * n_obs + src];
  out[(int64_t)c * n_cols + i] = v;
}

// thr^2 with room for the rounding of the square and of the root; infinity where thr^2 would
// lose its precision
double ob_bound(double thr) {
  return (thr > 1e-140 && thr < 1e140) ? thr * thr * 1.0000001 : INFINITY;
}

}  // namespace
}  // namespace onepose

using namespace onepose;

extern "C" {

int onepose_objbuild_version(void) { return 1; }

int onepose_filter_points(const double* xyz, const int* track_len, int n, int min_track,
                          const double* corners, float* xyz_out, int* index_out, int* count,
                          void* stream) {
  clear_error();
  OP_REQUIRE(n >= 1 && n <= kObMaxFilter, "filter_points: n=%d outside 1..%d", n, kObMaxFilter);
  OP_REQUIRE(xyz && xyz_out && index_out && count, "filter_points: null pointer");
  hipLaunchKernelGGL(ob_filter_kernel, dim3(1), dim3(kObScanThreads), 0,
                     static_cast<hipStream_t>(stream), xyz, track_len, n, min_track, corners,
                     xyz_out, index_out, count);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

int onepose_radius_neighbours(const void* xyz, int xyz_dtype, int n, double thr, int* row_start,
                              int* cols, int64_t cols_capacity, int64_t* info, void* stream) {
  clear_error();
  OP_REQUIRE(xyz_dtype == ONEPOSE_OBJ_F32 || xyz_dtype == ONEPOSE_OBJ_F64,
             "radius_neighbours: xyz_dtype=%d", xyz_dtype);
  OP_REQUIRE(n >= 1 && n <= kObMaxPoints, "radius_neighbours: n=%d outside 1..%d", n, kObMaxPoints);
  OP_REQUIRE(thr > 0.0 && thr < INFINITY, "radius_neighbours: the threshold is not positive and finite");
  OP_REQUIRE(cols_capacity >= 0 && cols_capacity <= (int64_t)INT_MAX,
             "radius_neighbours: cols_capacity=%lld outside 0..2^31-1", (long long)cols_capacity);
  OP_REQUIRE(xyz && row_start && info && (cols || cols_capacity == 0),
             "radius_neighbours: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double bound = ob_bound(thr);
  const dim3 grid(ceil_div(n, 4)), block(256);
  if (xyz_dtype == ONEPOSE_OBJ_F32)
    hipLaunchKernelGGL(ob_count_kernel<float>, grid, block, 0, st, static_cast<const float*>(xyz),
                       n, thr, bound, row_start);
  else
    hipLaunchKernelGGL(ob_count_kernel<double>, grid, block, 0, st,
                       static_cast<const double*>(xyz), n, thr, bound, row_start);
  OP_LAUNCHED();
  hipLaunchKernelGGL(ob_scan_kernel, dim3(1), dim3(kObScanThreads), 0, st, row_start, n,
                     cols_capacity, info);
  OP_LAUNCHED();
  if (cols_capacity == 0) return ONEPOSE_OK;   // a size query: info[0] is the needed capacity
  if (xyz_dtype == ONEPOSE_OBJ_F32)
    hipLaunchKernelGGL(ob_fill_kernel<float>, grid, block, 0, st, static_cast<const float*>(xyz),
                       n, thr, bound, row_start, info, cols);
  else
    hipLaunchKernelGGL(ob_fill_kernel<double>, grid, block, 0, st,
                       static_cast<const double*>(xyz), n, thr, bound, row_start, info, cols);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

int onepose_merge_greedy(const void* xyz, int xyz_dtype, int n, const int* row_start,
                         const int* cols, int* cluster_of, int* member_start, int* members,
                         double* mean, int* info, void* stream) {
  clear_error();
  OP_REQUIRE(xyz_dtype == ONEPOSE_OBJ_F32 || xyz_dtype == ONEPOSE_OBJ_F64,
             "merge_greedy: xyz_dtype=%d", xyz_dtype);
  OP_REQUIRE(n >= 1 && n <= kObMaxPoints, "merge_greedy: n=%d outside 1..%d", n, kObMaxPoints);
  OP_REQUIRE(xyz && row_start && cols && cluster_of && member_start && members && mean && info,
             "merge_greedy: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ob_fill_int_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, cluster_of, n,
                     -1);
  OP_LAUNCHED();
  if (xyz_dtype == ONEPOSE_OBJ_F32)
    hipLaunchKernelGGL(ob_merge_kernel<float>, dim3(1), dim3(64), 0, st,
                       static_cast<const float*>(xyz), n, row_start, cols, cluster_of,
                       member_start, members, mean, info);
  else
    hipLaunchKernelGGL(ob_merge_kernel<double>, dim3(1), dim3(64), 0, st,
                       static_cast<const double*>(xyz), n, row_start, cols, cluster_of,
                       member_start, members, mean, info);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

int onepose_lift_descriptors(const float* bank, int64_t bank_numel, const int64_t* block_offset,
                             const int* block_cols, int n_blocks, const int* obs_block,
                             const int* obs_feat, int n_obs, const int* seg_len, int n3, int dim,
                             int* seg_start, double* collected, double* mean64, float* mean32,
                             int* info, void* stream) {
  clear_error();
  OP_REQUIRE(dim >= 1 && dim <= kObMaxDim, "lift_descriptors: dim=%d outside 1..%d", dim, kObMaxDim);
  OP_REQUIRE(n_obs >= 1 && n_obs <= kObMaxObs, "lift_descriptors: n_obs=%d outside 1..2^28", n_obs);
  OP_REQUIRE(n3 >= 1 && n3 <= n_obs, "lift_descriptors: n3=%d outside 1..n_obs (no empty segment)",
             n3);
  OP_REQUIRE(n_blocks >= 1 && n_blocks <= (1 << 20), "lift_descriptors: n_blocks=%d", n_blocks);
  OP_REQUIRE(bank_numel >= 1, "lift_descriptors: bank_numel=%lld", (long long)bank_numel);
  OP_REQUIRE(bank && block_offset && block_cols && obs_block && obs_feat && seg_len && seg_start &&
                 collected && mean64 && mean32 && info,
             "lift_descriptors: null pointer");
  ObLift a{bank, bank_numel, block_offset, block_cols, n_blocks, obs_block, obs_feat, n_obs,
           seg_len, n3, dim, seg_start, collected, mean64, mean32, info};
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ob_lift_check_kernel, dim3(1), dim3(kObScanThreads), 0, st, a);
  OP_LAUNCHED();
  hipLaunchKernelGGL(ob_lift_kernel, dim3(ceil_div(n3, 64), ceil_div(dim, 4)), dim3(64, 4), 0, st,
                     a);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

int onepose_gather_leaves(const double* collected, int n_obs, int dim, const int64_t* cols,
                          int n_cols, float* out, void* stream) {
  clear_error();
  OP_REQUIRE(dim >= 1 && dim <= kObMaxDim, "gather_leaves: dim=%d outside 1..%d", dim, kObMaxDim);
  OP_REQUIRE(n_obs >= 1 && n_obs <= kObMaxObs, "gather_leaves: n_obs=%d outside 1..2^28", n_obs);
  OP_REQUIRE(n_cols >= 1 && n_cols <= kObMaxObs, "gather_leaves: n_cols=%d outside 1..2^28", n_cols);
  OP_REQUIRE(collected && cols && out, "gather_leaves: null pointer");
  hipLaunchKernelGGL(ob_leaves_kernel, dim3(ceil_div(n_cols, 64), ceil_div(dim, 4)), dim3(64, 4),
                     0, static_cast<hipStream_t>(stream), collected, n_obs, dim, cols, n_cols, out);
  OP_LAUNCHED();
  return ONEPOSE_OK;
}

}  // extern "C"
