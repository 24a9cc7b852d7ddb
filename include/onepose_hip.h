/*
 * onepose_hip.h -- C-ABI of libonepose_hip.so, the MI355X (gfx950) engine for OnePose's
 * GATsSPG 2D-3D matching + RANSAC-EPnP hot path.
 *
 * Plain pointers and sizes only.  Conventions:
 *   - every buffer belongs to the caller; the launch entry points never allocate or free
 *     device memory and never synchronise, so they are hipGraph-capturable (the measurement
 *     hooks onepose_profile_* are the exception: they own their timing buffers);
 *   - "device" pointers are HIP device memory (e.g. torch tensors' data_ptr()),
 *     "host" pointers are ordinary CPU memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *   - every function returns ONEPOSE_OK (0) or an error code, with a thread-local message
 *     in onepose_last_error(); no C++ exception crosses the ABI.
 *
 * The reference (huanghaoran111/OnePose @ /root/reference) has no FFI of its own: its hot
 * path is PyTorch + OpenCV called from Python.  Each entry point below names the
 * reference interface it replaces; INTEGRATION.md shows the ctypes binding
 * (onepose_amd/_lib.py) that a maintainer would drop in.
 */
#ifndef ONEPOSE_HIP_H
#define ONEPOSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  ONEPOSE_OK = 0,
  ONEPOSE_ERR_INVALID = 1,      /* bad argument / shape                                  */
  ONEPOSE_ERR_HIP = 2,          /* a HIP runtime call failed                            */
  ONEPOSE_ERR_UNSUPPORTED = 3,  /* valid in the reference, not supported by this build  */
  ONEPOSE_ERR_WORKSPACE = 4     /* workspace too small                                  */
};

/* Matcher arithmetic (onepose_match_ex / onepose_match_prepared_ex). */
enum {
  ONEPOSE_PREC_FP32 = 0,        /* every contraction on fp32-input MFMA: the reference's
                                   numerics up to summation order (bit-exact indices)   */
  ONEPOSE_PREC_BF16_ATTN = 1,   /* the attention layers' GEMMs (q/k/v projection, merge+MLP)
                                   take bf16-rounded operands on v_mfma_f32_32x32x16_bf16
                                   with fp32 accumulation (BASELINE config 5); GAT, final
                                   projection, scores and dual softmax stay fp32       */
  ONEPOSE_PREC_FP32_SPLIT = 2   /* every GEMM in fp32 by an exact 3-way bf16 split of both
                                   operands (x = hi + mid + lo) and the six bf16 MFMA
                                   products a_i b_j with i + j <= 2, fp32 accumulation:
                                   fp32-accurate (the dropped terms are < 2^-22 |a b|)  */
};

/* Descriptor element types of the _dt entry points (ABI 4).  The reference upcasts every
 * descriptor input with .float() (GATs_SuperGlue.py:219-221); an fp16 input is converted as it
 * is loaded, so the results are those of the fp32 path on the upcast inputs, bit for bit, and
 * the inputs (the object's leaves above all) take half the bytes in HBM. */
enum { ONEPOSE_DT_F32 = 0, ONEPOSE_DT_F16 = 1 };

/* Thread-local description of the last error ("" when none). */
const char* onepose_last_error(void);
/* ABI version, bumped on any signature change or new entry point (4: the per-precision
 * workspace and object-cache size queries; 5: the object cache's device-side header and
 * onepose_device_errors; 6: onepose_match_cached_stages; 7:
 * onepose_match_workspace_region; 8: onepose_pnp_max_points; 9: onepose_superpoint_layer). */
int onepose_abi_version(void);
/* (ABI 5) The library's sticky device-side error bits (ONEPOSE_DEVERR_*), set by kernels that
 * cannot return a status: *bits receives them, and `clear` != 0 resets them.  Synchronises with
 * the device (a host query; never call it inside a graph capture). */
enum {
  ONEPOSE_DEVERR_STALE_CACHE = 1   /* a cached forward found its object cache's header not the
                                    * one onepose_object_prepare wrote there (the memory was
                                    * freed and reused); that forward reported no match */
};
int onepose_device_errors(int clear, unsigned* bits);

/* ------------------------------------------------------------------------------------ *
 * GATsSPG matcher  --  replaces GATsSuperGlue.forward
 *   (src/models/GATsSPG_architectures/GATs_SuperGlue.py:203-278, reached from
 *    LitModelGATsSPG.forward, src/models/GATsSPG_lightning_model.py:36-37, and
 *    inference.py:146)
 * ------------------------------------------------------------------------------------ */

/* Number of weight tensors the packer consumes, and the reference state-dict key of
 * tensor i (e.g. "gnn.layers.1.attn.proj.0.weight").  The unused kenc_2d / kenc_3d /
 * bin_score entries (never read by forward, GATs_SuperGlue.py:172-201) are not listed. */
int onepose_matcher_num_tensors(void);
const char* onepose_matcher_tensor_name(int i);
/* Element count tensor i must have. */
int64_t onepose_matcher_tensor_numel(int i);

/* Bytes of the packed weight panel. */
size_t onepose_matcher_packed_bytes(void);

/* Pack the float32 host tensors (in onepose_matcher_tensor_name order) into the
 * device-ready panel `packed_host` (onepose_matcher_packed_bytes() bytes, host memory).
 * Packing permutes the q/k/v projections to head-major channel order, folds the GAT
 * attention vectors through W (h.(W a) == (h W).a, GATs.py:68-69,113-115) and lays the
 * matrices out as [out][in].  Upload the panel to the device once; it is read-only. */
int onepose_matcher_pack(const float* const* tensors, int n_tensors, void* packed_host);

/* Workspace bytes onepose_match needs for this shape.  with_conf=0 adds room for the
 * score matrix that would otherwise live in `conf`. */
size_t onepose_match_workspace_bytes(int batch, int n1, int n3, int num_leaf, int with_conf);
/* (ABI 4) The same for one precision: fp32 needs no bf16 activation planes, so its workspace
 * is smaller (the query above is the largest over precisions and stays valid for all).  A
 * match call checks `workspace_bytes` against its own precision's need. */
size_t onepose_match_workspace_bytes_ex(int batch, int n1, int n3, int num_leaf, int with_conf,
                                        int precision);

/* One matcher forward over `batch` frames.
 *   desc2d  [batch, 256, n1]        descriptors2d_query  (device, fp32)
 *   desc3d  [batch, 256, n3]        descriptors3d_db     (device; bstride may be 0)
 *   leaves  [batch, 256, n3*L]      descriptors2d_db     (device; bstride may be 0)
 *   outputs matches0 [batch, n1] int64, matches1 [batch, n3] int64,
 *           mscores0 [batch, n1] fp32, mscores1 [batch, n3] fp32,
 *           conf [batch, n1, n3] fp32 or NULL (conf_matrix).
 * Batch strides are in elements.  n1, n3 >= 1 (the empty-input branch of
 * GATs_SuperGlue.py:223-231 is handled by the caller).  1 <= num_leaf <= 16. */
int onepose_match(const void* packed_weights,
                  const float* desc2d, int64_t desc2d_bstride,
                  const float* desc3d, int64_t desc3d_bstride,
                  const float* leaves, int64_t leaves_bstride,
                  int batch, int n1, int n3, int num_leaf,
                  float scale_factor, float match_threshold,
                  int64_t* matches0, int64_t* matches1,
                  float* mscores0, float* mscores1, float* conf,
                  void* workspace, size_t workspace_bytes, void* stream);

/* Per-object leaf preparation.  The GAT layers read the leaves point-major
 * ([n3][num_leaf][256]: one 3D point's leaves contiguous) -- onepose_match transposes its
 * reference-layout input into the workspace on every call; a caller that keeps one object
 * resident across frames (inference.py:89-90 uploads it per frame) can transpose once with
 * onepose_prepare_leaves and call onepose_match_prepared.
 *   leaves [batch, 256, n3*L] (bstride elements)  ->  out [batch, n3*L, 256]
 * onepose_match_prepared takes the same arguments as onepose_match with the prepared leaves
 * (prepared_bstride elements per sample, 0 = shared) and the same workspace size. */
size_t onepose_leaves_prepared_bytes(int batch, int n3, int num_leaf);
int onepose_prepare_leaves(const float* leaves, int64_t leaves_bstride, int batch, int n3,
                           int num_leaf, float* out, void* stream);
/* (ABI 4) leaves of `dtype` (ONEPOSE_DT_*); the prepared copy is fp32. */
int onepose_prepare_leaves_dt(const void* leaves, int dtype, int64_t leaves_bstride, int batch,
                              int n3, int num_leaf, float* out, void* stream);
/* The same two calls with a precision mode (ONEPOSE_PREC_*); the plain forms are
 * ONEPOSE_PREC_FP32. */
int onepose_match_ex(const void* packed_weights,
                     const float* desc2d, int64_t desc2d_bstride,
                     const float* desc3d, int64_t desc3d_bstride,
                     const float* leaves, int64_t leaves_bstride,
                     int batch, int n1, int n3, int num_leaf,
                     float scale_factor, float match_threshold, int precision,
                     int64_t* matches0, int64_t* matches1,
                     float* mscores0, float* mscores1, float* conf,
                     void* workspace, size_t workspace_bytes, void* stream);
/* (ABI 4) onepose_match_ex with desc2d, desc3d and leaves of `desc_dtype` (ONEPOSE_DT_*). */
int onepose_match_dt(const void* packed_weights,
                     const void* desc2d, int64_t desc2d_bstride,
                     const void* desc3d, int64_t desc3d_bstride,
                     const void* leaves, int64_t leaves_bstride, int desc_dtype,
                     int batch, int n1, int n3, int num_leaf,
                     float scale_factor, float match_threshold, int precision,
                     int64_t* matches0, int64_t* matches1,
                     float* mscores0, float* mscores1, float* conf,
                     void* workspace, size_t workspace_bytes, void* stream);
int onepose_match_prepared_ex(const void* packed_weights,
                              const float* desc2d, int64_t desc2d_bstride,
                              const float* desc3d, int64_t desc3d_bstride,
                              const float* leaves_prepared, int64_t prepared_bstride,
                              int batch, int n1, int n3, int num_leaf,
                              float scale_factor, float match_threshold, int precision,
                              int64_t* matches0, int64_t* matches1,
                              float* mscores0, float* mscores1, float* conf,
                              void* workspace, size_t workspace_bytes, void* stream);
int onepose_match_prepared(const void* packed_weights,
                           const float* desc2d, int64_t desc2d_bstride,
                           const float* desc3d, int64_t desc3d_bstride,
                           const float* leaves_prepared, int64_t prepared_bstride,
                           int batch, int n1, int n3, int num_leaf,
                           float scale_factor, float match_threshold,
                           int64_t* matches0, int64_t* matches1,
                           float* mscores0, float* mscores1, float* conf,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------ *
 * Per-object cache (SURVEY.md §8b ops_object_prepare, §8f rank 2).  Two parts of the forward
 * depend on the object alone: GAT layer 0 (GATs.py:62-123, the 3D descriptors and their
 * leaves) and the 3D half of self-attention 1 (GATs_SuperGlue.py:67-85 -- the 3D side attends
 * only to itself there).  onepose_object_prepare runs them once per object and leaves the
 * 3D state entering layer 2 in `cache` ([n3][256] fp32), followed by the leaf logits
 * leaf_j . (W a)_lo of GAT layers 1-3 ([3][n3][16] fp32; GATs.py:113, constant per object since
 * the leaves never change, GATs_SuperGlue.py:70-72) and by cross-attention 1's frame-
 * independent 3D half (layer 2, GATs_SuperGlue.py:74-78: the 3D side's phi(q), sum phi(k), the
 * 2D side's folded message weights and the W1a x half of its MLP conv 1) --
 * onepose_object_cache_bytes in all (an opaque layout); onepose_match_cached then runs every
 * frame from there.
 *
 * `flags` (ONEPOSE_OBJ_*) fix the cache's layout and contents at prepare time; pass the same
 * value to onepose_object_cache_bytes and onepose_match_cached.  With ONEPOSE_OBJ_GAT_TABLES and
 * num_leaf <= 8 the cache also holds prefix tables of GAT layers 1-3 (the leaves sorted by
 * logit, exp-weighted prefix and suffix sums: [3][n3][2 num_leaf][256] fp32 plus [3][n3][16]
 * sorted logits, i.e. 6 KB x num_leaf + 192 B per 3D point: 202 MB at n3 = 4096, L = 8), and a
 * cached frame's GAT layers 1-3 read two table rows per 3D point instead of its L leaves; they
 * then differ from computing the layers from the leaves in rounding only.  Without it (flags
 * 0; the tables are never built for num_leaf > 8) the results are bit-identical to
 * onepose_match_prepared_ex's on the same object (the same kernels and tiles produce the cached
 * state), provided the cache was prepared with the same `precision`.  Without tables the cache
 * is 4 KB + 192 B per 3D point (17.6 MB at n3 = 4096) plus a 0.75 MB fixed part.
 *   desc3d:          [256][n3] reference layout (descriptors3d_db of one object)
 *   leaves_prepared: [n3*L][256] point-major (onepose_prepare_leaves of the object)
 * The cache is shared by every sample of a batch (one object per call); it is read-only for
 * onepose_match_cached, so any number of streams may use one cache concurrently.
 *
 * The library records, per cache address, the (n3, num_leaf, precision, flags) that
 * onepose_object_prepare built it with (host-side; nothing is read back from the device).
 * onepose_match_cached returns ONEPOSE_ERR_INVALID for a cache it has no record of, or whose
 * record differs from its own arguments: the layout depends on n3, num_leaf and flags, and
 * the folded Mf weights are fp32 for ONEPOSE_PREC_FP32 and bf16 planes for the other
 * precisions, so a mismatched call would read the wrong bytes. A copy of a cache at another
 * address is therefore refused; prepare it there instead. onepose_object_release forgets a
 * cache's record (call it before the memory is freed, if the allocator may hand the address
 * to another cache that is not prepared again); a new onepose_object_prepare at the same
 * address replaces the record. onepose_object_cache_bytes returns 0 for flags that prepare
 * would refuse.
 * (ABI 5) The record cannot see memory that was freed and handed to something else at the
 * same address without onepose_object_release.  So the prepare also writes a 64-B header at
 * the end of the cache (its n3, num_leaf, precision, flags and a generation the record keeps),
 * and onepose_match_cached's first kernel compares it with the record on the device: a
 * mismatch makes that forward report no match (matches -1, scores 0) and sets
 * ONEPOSE_DEVERR_STALE_CACHE (onepose_device_errors) -- without a host synchronisation, so
 * graph-captured forwards keep the check.
 * ------------------------------------------------------------------------------------ */
enum {
  ONEPOSE_OBJ_GAT_TABLES = 1    /* build / use the GAT prefix tables (num_leaf <= 8)          */
};
size_t onepose_object_cache_bytes(int n3, int num_leaf, int flags);
/* (ABI 4) The cache bytes for one precision: the bf16 activation planes of the cached phi(q)
 * (1.5 KB per point) only in the bf16 modes.  A cache sized by this query must be prepared and
 * matched with that precision; onepose_object_cache_bytes fits every precision. */
size_t onepose_object_cache_bytes_ex(int n3, int num_leaf, int flags, int precision);
size_t onepose_object_prepare_workspace_bytes(int n3, int num_leaf);
int onepose_object_prepare(const void* packed_weights, const float* desc3d,
                           const float* leaves_prepared, int n3, int num_leaf, int precision,
                           int flags, float* cache, void* workspace, size_t workspace_bytes,
                           void* stream);
/* (ABI 4) desc3d [256, n3] of `desc_dtype` (ONEPOSE_DT_*). */
int onepose_object_prepare_dt(const void* packed_weights, const void* desc3d, int desc_dtype,
                              const float* leaves_prepared, int n3, int num_leaf, int precision,
                              int flags, float* cache, void* workspace, size_t workspace_bytes,
                              void* stream);
void onepose_object_release(const float* cache);
/* Workspace: onepose_match_workspace_bytes(batch, n1, n3, num_leaf, conf != NULL). */
int onepose_match_cached(const void* packed_weights,
                         const float* desc2d, int64_t desc2d_bstride,
                         const float* object_cache,
                         const float* leaves_prepared, int64_t prepared_bstride,
                         int batch, int n1, int n3, int num_leaf,
                         float scale_factor, float match_threshold, int precision,
                         int object_flags,
                         int64_t* matches0, int64_t* matches1,
                         float* mscores0, float* mscores1, float* conf,
                         void* workspace, size_t workspace_bytes, void* stream);
/* (ABI 4) desc2d [batch, 256, n1] of `desc_dtype` (ONEPOSE_DT_*). */
int onepose_match_cached_dt(const void* packed_weights,
                            const void* desc2d, int desc_dtype, int64_t desc2d_bstride,
                            const float* object_cache,
                            const float* leaves_prepared, int64_t prepared_bstride,
                            int batch, int n1, int n3, int num_leaf,
                            float scale_factor, float match_threshold, int precision,
                            int object_flags,
                            int64_t* matches0, int64_t* matches1,
                            float* mscores0, float* mscores1, float* conf,
                            void* workspace, size_t workspace_bytes, void* stream);
/* (ABI 6) onepose_match_cached_dt as a range of its stages, for a caller that pipelines frames
 * through buffer slots (one workspace per slot) and wants stages off the matcher's launch
 * chain.  The forward's stages, in order:
 *   ONEPOSE_STAGE_INPUTS        its first kernel: desc2d into the workspace's token-major layout,
 *                               the workspace's arrival counters zeroed, the object cache's
 *                               header checked;
 *   ONEPOSE_STAGE_LAYER0 + i    GNN layer i, i = 0..11 of ['GATs', 'self', 'cross'] x 4
 *                               (GATs_SuperGlue.py:184-191; the cached object supplies GAT 0 and
 *                               the 3D half of self-attention 1);
 *   ONEPOSE_STAGE_FINAL         the final projection (+ L2 normalisation) of both sides;
 *   ONEPOSE_STAGE_SCORE         the score GEMM (S and its softmax partials in the workspace, or
 *                               S in `conf`);
 *   ONEPOSE_STAGE_WINNERS       the dual softmax's winners and the mutual check (matches /
 *                               scores, and conf when requested).
 * onepose_match_cached_stages runs stages first_stage..last_stage.  Consecutive ranges of one
 * forward, run in order with the same arguments (on one stream or ordered by events), give the
 * bits of one onepose_match_cached_dt call (the range INPUTS..WINNERS); nothing else may use
 * the workspace in between.  So the input stage may run as soon as the workspace's previous
 * forward has finished -- e.g. on the stream of that forward's pose stage -- and the last
 * stages on the pose stream of their own frame. */
enum { ONEPOSE_STAGE_INPUTS = 0, ONEPOSE_STAGE_LAYER0 = 1, ONEPOSE_STAGE_FINAL = 13,
       ONEPOSE_STAGE_SCORE = 14, ONEPOSE_STAGE_WINNERS = 15 };
int onepose_match_cached_stages(const void* packed_weights,
                                const void* desc2d, int desc_dtype, int64_t desc2d_bstride,
                                const float* object_cache,
                                const float* leaves_prepared, int64_t prepared_bstride,
                                int batch, int n1, int n3, int num_leaf,
                                float scale_factor, float match_threshold, int precision,
                                int object_flags,
                                int64_t* matches0, int64_t* matches1,
                                float* mscores0, float* mscores1, float* conf,
                                void* workspace, size_t workspace_bytes, int first_stage,
                                int last_stage, void* stream);

/* (ABI 7) Where a stage of onepose_match_cached_stages leaves its result, for a caller (a
 * test) that runs the forward a stage at a time and reads the workspace in between.  A
 * host-side query: no device call.  For a forward of this shape (with_conf: conf != NULL) and
 * precision, after the stages INPUTS..after_stage have run, `region` is
 *   ONEPOSE_REGION_STATE2D / _STATE3D   the 2D / 3D token state, [batch][n][256] fp32 (the GNN
 *                                       layers alternate between two buffers per side, so the
 *                                       answer depends on after_stage);
 *   ONEPOSE_REGION_DESC2D / _DESC3D     the projected, L2-normalised descriptors,
 *                                       [batch][n][256] fp32 (after_stage >= ONEPOSE_STAGE_FINAL,
 *                                       ONEPOSE_ERR_INVALID before).
 * *where = ONEPOSE_WHERE_WORKSPACE: *bytes bytes at *offset bytes into the workspace.
 * *where = ONEPOSE_WHERE_OBJECT_CACHE (the 3D state up to ONEPOSE_STAGE_LAYER0 + 1: GAT 0 and the
 * 3D half of self-attention 1 are the object's): the first n3*256 floats of the object cache,
 * "the 3D state entering layer 2", [n3][256] shared by the batch; *offset = 0.
 * The score matrix needs no query: after ONEPOSE_STAGE_SCORE with a conf buffer S is in conf,
 * after ONEPOSE_STAGE_WINNERS conf holds conf_matrix. */
enum { ONEPOSE_REGION_STATE2D = 0, ONEPOSE_REGION_STATE3D = 1, ONEPOSE_REGION_DESC2D = 2,
       ONEPOSE_REGION_DESC3D = 3 };
enum { ONEPOSE_WHERE_WORKSPACE = 0, ONEPOSE_WHERE_OBJECT_CACHE = 1 };
int onepose_match_workspace_region(int batch, int n1, int n3, int num_leaf, int with_conf,
                                   int precision, int region, int after_stage, int* where,
                                   size_t* offset, size_t* bytes);

/* ------------------------------------------------------------------------------------ *
 * N3-sharded single frame (SURVEY.md §8e optional / §8f rank 4): one frame's 3D points split
 * over `world` ranks (one process per GPU), rank r holding points [start_r, start_r + count_r)
 * with start_r = floor(n3_total * r / world) (onepose_shard_range).  Every rank holds the
 * whole 2D side.  Per attention layer the 3D side's KV / sum phi(k) and its InstanceNorm
 * (n, mean, M2) cross ranks; after the score GEMM the row softmax statistics, the row winners
 * and the column winners do -- each as an all-gather of one fixed-size block per rank,
 * merged in rank order on the device.  The caller supplies the exchange buffers (send: one
 * block of xchg_bytes, recv: world blocks) and a callback that, for `bytes_per_rank` <=
 * xchg_bytes, makes recv hold every rank's first `bytes_per_rank` bytes of send (rank-major,
 * block stride = bytes_per_rank) ordered on `stream` (an RCCL all-gather enqueued there, or a
 * synchronous exchange); it returns 0 on success.
 * Inputs: desc2d [batch,256,n1]; desc3d_shard [batch,256,count_r]; the shard's leaves
 * prepared point-major (onepose_prepare_leaves on the shard).  Outputs on every rank, for the
 * whole frame: matches0 / mscores0 [batch,n1], matches1 / mscores1 [batch,n3_total] (indices
 * global); conf_shard [batch,n1,count_r] optional.
 * ------------------------------------------------------------------------------------ */
typedef int (*onepose_allgather_fn)(size_t bytes_per_rank, void* stream, void* user);
void onepose_shard_range(int n3_total, int world, int rank, int* start, int* count);
size_t onepose_match_sharded_xchg_bytes(int batch, int n1, int n3_total, int world);
size_t onepose_match_sharded_workspace_bytes(int batch, int n1, int n3_total, int world, int rank,
                                             int num_leaf, int with_conf);
int onepose_match_sharded(const void* packed_weights,
                          const float* desc2d, int64_t desc2d_bstride,
                          const float* desc3d_shard, int64_t desc3d_bstride,
                          const float* leaves_shard_prepared, int64_t prepared_bstride,
                          int batch, int n1, int n3_total, int num_leaf, int world, int rank,
                          float scale_factor, float match_threshold, int precision,
                          void* xchg_send, void* xchg_recv, size_t xchg_bytes,
                          onepose_allgather_fn allgather, void* user,
                          int64_t* matches0, int64_t* matches1,
                          float* mscores0, float* mscores1, float* conf_shard,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------ *
 * SuperPoint descriptor sampling  --  replaces sample_descriptors
 *   (src/models/extractors/SuperPoint/superpoint.py:95-113)
 * keypoints [batch, n, 2] (x, y) pixels, dense [batch, c, h, w] -> out [batch, c, n],
 * bilinear, zero padding, L2-normalised over c.  align_corners mirrors the reference's
 * torch-version switch (superpoint.py:108).  All device pointers.
 * ------------------------------------------------------------------------------------ */
int onepose_sample_descriptors(const float* keypoints, const float* dense,
                               int batch, int n, int c, int h, int w, int s,
                               int align_corners, float* out, void* stream);

/* ------------------------------------------------------------------------------------ *
 * Correspondence selection  --  replaces the host-side masking of inference.py:147-152
 *   (valid = matches > -1; mkpts2d = kpts2d[valid]; mkpts3d = kpts3d[matches[valid]])
 * plus the float64 scaling + float32 conversion solvePnPRansac applies to its inputs
 *   (eval_utils.py:22-26).
 * matches0 [batch, n1] int64, kpts2d [batch, n1, 2] fp32, kpts3d [batch, n3, 3] fp32
 * (kpts3d bstride may be 0) -> pts2d [batch, n1, 2], pts3d [batch, n1, 3] fp32 compacted
 * in ascending 2D index order, counts [batch] int32.  All device pointers.
 * ------------------------------------------------------------------------------------ */
int onepose_select_correspondences(const int64_t* matches0, const float* kpts2d,
                                   int64_t kpts2d_bstride, const float* kpts3d,
                                   int64_t kpts3d_bstride, int batch, int n1, int n3,
                                   double scale3d, float* pts2d, float* pts3d, int* counts,
                                   void* stream);

/* ------------------------------------------------------------------------------------ *
 * Batched RANSAC-EPnP  --  replaces ransac_PnP (src/utils/eval_utils.py:18-42), i.e.
 *   cv2.solvePnPRansac(pts3d*scale, pts2d, K, 0, reprojectionError, iterationsCount,
 *                      flags=SOLVEPNP_EPNP) + Rodrigues + tvec/scale,
 * restated after OpenCV 4.4's solvePnPRansac / RANSACPointSetRegistrator / epnp
 * (same cv::RNG stream, same subset rule, same adaptive iteration count, final EPnP refit
 * on the inliers).  One frame per batch entry; frames are independent.
 *   pts2d [batch, max_points, 2], pts3d [batch, max_points, 3] fp32 (already scaled),
 *   counts [batch] int32, K [batch, 9] fp64 row-major (K_bstride may be 0).
 * Outputs: pose34 [batch, 12] fp64 row-major [R | t/scale], inlier_mask
 * [batch, max_points] uint8, n_inliers [batch] int32, status [batch] int32:
 *   0 = solved; 1 = fewer than 4 points (reference: cv2.error -> identity pose, no inliers);
 *   2 = RANSAC found no model (identity pose, no inliers);
 * Exactly 4 points follow solvePnPRansac's P3P branch: the P3P kernel (Gao) decides model / no
 * model (status 2), the pose is the EPnP refit over all four.
 * A 5-point EPnP (every RANSAC hypothesis) has a two-dimensional null space; its basis, which
 * an SVD leaves arbitrary, is made canonical so that a model is a function of its five points.
 * All device pointers.
 * (ABI 8) max_points is limited by the 160 KB of LDS a workgroup can hold: the solver keeps
 * its state and the frame's points (20 B each) there.  onepose_pnp_max_points() is the largest
 * max_points (and the largest n1 of onepose_pose_stage) that fits, a host-side query; a larger
 * one is refused with ONEPOSE_ERR_INVALID before anything is launched.
 * ------------------------------------------------------------------------------------ */
int onepose_pnp_max_points(void);
size_t onepose_pnp_workspace_bytes(int batch, int max_points, int max_iters);
int onepose_pnp_ransac(const float* pts2d, const float* pts3d, const int* counts,
                       int max_points, const double* K, int64_t K_bstride, int batch,
                       double scale, float reproj_error, int max_iters, double confidence,
                       double* pose34, uint8_t* inlier_mask, int* n_inliers, int* status,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------ *
 * cm/deg pose error  --  replaces query_pose_error (src/utils/eval_utils.py:45-63) and
 * Evaluator.cm_degree_*_metric (src/evaluators/cmd_evaluator.py:11-31).
 * pose_pred [batch, 12], pose_gt [batch, 12] fp64 row-major 3x4 (gt bstride may be 0)
 * -> R_err_deg [batch], t_err_cm [batch] fp64, cmd [batch, 3] uint8 for 1/3/5 cm-deg.
 * ------------------------------------------------------------------------------------ */
int onepose_pose_errors(const double* pose_pred, const double* pose_gt, int64_t gt_bstride,
                        int batch, double* R_err_deg, double* t_err_cm, uint8_t* cmd,
                        void* stream);

/* ------------------------------------------------------------------------------------ *
 * The whole per-frame pose stage in two launches  --  inference.py:147-160 (mkpts selection,
 * ransac_PnP, evaluator.evaluate): onepose_select_correspondences fused into the RANSAC
 * kernel (which compacts the matches straight into its LDS copy of the points) and
 * onepose_pose_errors fused into the refit kernel.  Same results as the three calls, with
 * max_points = n1 (pts2d [batch, n1, 2], pts3d [batch, n1, 3], inlier_mask [batch, n1]).
 * scale multiplies kpts3d (select) and divides the translation (ransac_PnP), as inference.py
 * uses one scale for both.  pose_gt null: no error outputs (R_err_deg / t_err_cm / cmd may
 * be null).  Workspace: onepose_pnp_workspace_bytes(batch, n1, max_iters).
 * ------------------------------------------------------------------------------------ */
int onepose_pose_stage(const int64_t* matches0, const float* kpts2d, int64_t kpts2d_bstride,
                       const float* kpts3d, int64_t kpts3d_bstride, int batch, int n1, int n3,
                       double scale, const double* K, int64_t K_bstride, float reproj_error,
                       int max_iters, double confidence, const double* pose_gt,
                       int64_t gt_bstride, float* pts2d, float* pts3d, int* counts,
                       double* pose34, uint8_t* inlier_mask, int* n_inliers, int* status,
                       double* R_err_deg, double* t_err_cm, uint8_t* cmd, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------ *
 * SuperPoint keypoint detector + descriptor -- replaces SuperPoint.forward
 * (src/models/extractors/SuperPoint/superpoint.py:170-224; the model extract_features.py:
 * 27-40 builds, nms_radius 3, keypoint_threshold 0.005, remove_borders 4, max_keypoints
 * 4096 there).  Weights: the 24 tensors conv1a.weight, conv1a.bias, ... convDb.bias in
 * onepose_superpoint_tensor_name order, torch layouts ([cout][cin][k][k], [cout]), packed
 * host-side into onepose_superpoint_packed_bytes() bytes (then copied to the device).
 * image [batch][h][w] fp32 in [0,1] (h, w multiples of 8).  Outputs, per sample b:
 *   keypoints [batch][max_keypoints][2] (x, y), scores [batch][max_keypoints],
 *   descriptors [batch][256][max_keypoints], counts [batch] -- the first counts[b] entries
 *   are the reference's keypoints in its order (raster order when at most max_keypoints
 *   survive NMS + threshold + borders, torch.topk's descending order otherwise); the rest
 *   are zero.  score_map [batch][h][w] and dense_desc [batch][h/8][w/8][256] (normalised)
 *   are optional (may be null).  nms_radius <= 8; max_keypoints in [1, 16384], or >= h*w
 * (the reference's -1: every pixel, no top-k).
 * ------------------------------------------------------------------------------------ */
int onepose_superpoint_num_tensors(void);
const char* onepose_superpoint_tensor_name(int i);
size_t onepose_superpoint_packed_bytes(void);
int onepose_superpoint_pack(const float* const* tensors, int n_tensors, void* packed_host);
size_t onepose_superpoint_workspace_bytes(int batch, int h, int w);
int onepose_superpoint(const void* packed, const float* image, int batch, int h, int w,
                       int nms_radius, float keypoint_threshold, int remove_borders,
                       int max_keypoints, int align_corners, float* keypoints, float* scores,
                       float* descriptors, int* counts, float* score_map, float* dense_desc,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The detector's tail alone -- simple_nms, threshold, remove_borders, top_k_keypoints, the
 * (y,x)->(x,y) flip and sample_descriptors (superpoint.py:47-113, 181-243) -- from a score
 * map [batch][h][w] (softmax + pixel shuffle, before NMS) and a normalised dense descriptor
 * map [batch][h/8][w/8][256].  Outputs and limits as onepose_superpoint. */
size_t onepose_superpoint_detect_workspace_bytes(int batch, int h, int w);
int onepose_superpoint_detect(const float* score_map, const float* dense_desc, int batch, int h,
                              int w, int nms_radius, float keypoint_threshold, int remove_borders,
                              int max_keypoints, int align_corners, float* keypoints,
                              float* scores, float* descriptors, int* counts, void* workspace,
                              size_t workspace_bytes, void* stream);
/* (ABI 9) One convolution layer of the network alone, for stage-by-stage checks: layer 0 =
 * conv1a .. 11 = convDb (onepose_superpoint_tensor_name order), launched exactly as
 * onepose_superpoint launches it -- the same kernel, tile, fused 2x2 max-pool (layers 1, 3, 5)
 * and epilogue (ReLU; softmax over 65 + pixel shuffle for convPb; bias only for convDb).
 * h, w are the layer's input map size (any >= 1 with h * w * 256 < 2^31; even for the pooled
 * layers).  x is NHWC
 * [batch][h][w][cin] ([batch][h][w] for layer 0); y receives NHWC [batch][h][w][cout],
 * [batch][h/2][w/2][cout] for a pooled layer, or the score map [batch][8h][8w] for layer 9:
 * onepose_superpoint_layer_out_floats(layer, h, w) floats per sample (0 for a refused
 * layer or size).  All device pointers. */
size_t onepose_superpoint_layer_out_floats(int layer, int h, int w);
int onepose_superpoint_layer(const void* packed, int layer, const float* x, int batch, int h,
                             int w, float* y, void* stream);

/* ------------------------------------------------------------------------------------ *
 * SuperGlue 2D-2D matcher  --  replaces SuperGlue.forward
 *   (src/models/matchers/SuperGlue/superglue.py:264-327: the keypoint encoder, 18 softmax
 *    attention layers, the final projection, log_optimal_transport and the mutual check;
 *    reached from inference_demo.py's LocalFeatureObjectDetector and src/sfm/match_features.py)
 * fp32 only.  This family is versioned on its own: onepose_superglue_version() returns 1 and
 * is bumped when one of the entry points below changes; onepose_abi_version() was not bumped
 * for it -- nothing that existed at ABI 8 changed, and a caller of the GATsSPG / pose entry points need
 * not rebuild for a matcher it does not use.
 * ------------------------------------------------------------------------------------ */
int onepose_superglue_version(void);
/* The packer, as the GATsSPG matcher's: tensor i's reference state-dict key (the BatchNorm
 * weight / bias / running_mean / running_var and bin_score included; num_batches_tracked is
 * not consumed) and element count; float32 host tensors in that order -> one device-ready
 * panel.  Packing folds each eval-mode BatchNorm into the convolution before it, permutes
 * q/k/v (and the merge convolution's inputs) to head-major channels (the reference's
 * .view(B, 64, 4, N) makes channel c = d*4 + h) and folds the merge convolution into the
 * message half of MLP conv 1. */
int onepose_superglue_num_tensors(void);
const char* onepose_superglue_tensor_name(int i);
int64_t onepose_superglue_tensor_numel(int i);
size_t onepose_superglue_packed_bytes(void);
int onepose_superglue_pack(const float* const* tensors, int n_tensors, void* packed_host);
/* Workspace bytes of one forward (0 for a shape the forward refuses). */
size_t onepose_superglue_workspace_bytes(int batch, int n0, int n1);
/* One forward over `batch` pairs.  Per image i: desc_i [batch, 256, n_i], kpts_i [batch, n_i, 2]
 * (x, y pixels), scores_i [batch, n_i], each with a batch stride in elements; stride 0 = the
 * tensor is shared by the batch (one query against many views).  h_i, w_i: the image sizes
 * normalize_keypoints reads (:67-84).  sinkhorn_iters >= 0 and match_threshold are the
 * reference's config entries.  precision: ONEPOSE_PREC_FP32 only (others:
 * ONEPOSE_ERR_UNSUPPORTED).  Outputs matches0 [batch, n0] / matches1 [batch, n1] int64 (-1 = no
 * match), mscores0 / mscores1 fp32; log_assignment [batch, n0+1, n1+1] fp32 or NULL: the
 * reference's `scores` after log_optimal_transport.  1 <= n0, n1 <= 16384 (the caller handles
 * the empty branch, :269-276).  All device pointers; the workspace 256-byte aligned. */
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
                            size_t workspace_bytes, void* stream);
/* log_optimal_transport alone (:190-210): scores [batch, m, n] (bstride elements) with the
 * dustbin score alpha -> out [batch, m+1, n+1] = Z + u + v - norm after `iters` >= 0 log-space
 * Sinkhorn iterations.  Deterministic: no atomics, every merge in a fixed order. */
size_t onepose_log_optimal_transport_workspace_bytes(int batch, int m, int n);
int onepose_log_optimal_transport(const float* scores, int64_t scores_bstride, int batch, int m,
                                  int n, float alpha, int iters, float* out, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* Multi-head softmax attention alone (:103-119): q [batch, n, 256], k, v [batch, m, 256],
 * token-major with head-major channels (4 heads x 64) -> out [batch, n, 256] =
 * softmax(q k^T / 8) v per head.  Batch strides in elements (multiples of 4; 0 = shared input);
 * pointers 16-byte aligned. */
int onepose_mha_softmax(const float* q, int64_t q_bstride, const float* k, int64_t k_bstride,
                        const float* v, int64_t v_bstride, int batch, int n, int m, float* out,
                        int64_t out_bstride, void* stream);

/* ------------------------------------------------------------------------------------ *
 * 2D object detector  --  replaces the arithmetic of LocalFeatureObjectDetector
 *   (src/local_feature_2D_detector/local_feature_2D_detector.py: match_worker :77-133,
 *    detect_by_matching :135-147, crop_img_by_bbox :160-186), the caller the SuperGlue family
 *   above was built for: after the SuperGlue forwards of one query frame against the reference
 *   views, the correspondence selection, cv2.estimateAffinePartial2D per view, the box of the
 *   warped view corners, the choice of view and the two cv2.warpAffine crops.
 * This family is versioned on its own, as the SuperGlue family: onepose_detector_version()
 * returns 1; onepose_abi_version() was not bumped for it.
 * OpenCV is restated after 4.4's ptsetreg.cpp / imgwarp.cpp from its published algorithm (no
 * OpenCV here): parity with cv2 itself is pinned only by known-answer scenes.
 * ------------------------------------------------------------------------------------ */
int onepose_detector_version(void);
/* cv2.estimateAffinePartial2D(from, to, method=RANSAC, ransacReprojThreshold=threshold,
 * maxIters=max_iters, confidence, refineIters=refine_iters), one view per batch entry (one
 * workgroup each, the view's points in LDS at 16 B per point): RANSACPointSetRegistrator with
 * two-point subsets drawn from cv::RNG((uint64)-1), the minimal similarity in double, float32
 * errors against (float)(threshold^2), RANSACUpdateNumIters, then Levenberg-Marquardt over the
 * inliers (the mask is not recomputed).
 *   from, to [batch, max_points, 2] fp32, counts [batch] int32 (clamped to [0, max_points]).
 * Outputs: affine [batch, 6] fp64 row-major [a -b tx; b a ty] (zeros without an estimate),
 * inlier_mask [batch, max_points] uint8, n_inliers [batch] int32, status [batch] int32:
 *   0 = solved; 1 = fewer than 2 points; 2 = RANSAC found no model (every subset drawn had
 *   coincident source points, or no model reached 2 inliers).
 * Exactly 2 points: the minimal model of the two, both inliers, no refinement.
 * onepose_affine_partial_max_points(): the largest max_points that fits the 160 KB of LDS (a
 * host-side query); a larger one is refused with ONEPOSE_ERR_INVALID before anything is
 * launched.  Workspace: onepose_affine_partial_workspace_bytes(batch, max_points); after the
 * call its first `batch` int32 hold each view's number of RANSAC iterations run.
 * All device pointers. */
int onepose_affine_partial_max_points(void);
size_t onepose_affine_partial_workspace_bytes(int batch, int max_points);
int onepose_affine_partial_ransac(const float* from, const float* to, const int* counts,
                                  int max_points, int batch, double threshold, int max_iters,
                                  double confidence, int refine_iters, double* affine,
                                  uint8_t* inlier_mask, int* n_inliers, int* status,
                                  void* workspace, size_t workspace_bytes, void* stream);
/* match_worker + detect_by_matching for one query frame, in one launch per frame plus one
 * small ranking launch.  View b: matches0 [batch, n0] int64 (SuperGlue's, view keypoint ->
 * query keypoint, -1 = none), of which the first counts0[b] are read (counts0 null: all n0);
 * kpts0 [batch, n0, 2] the views' keypoints, kpts1 [n1, 2] the query's (kpts1_bstride
 * elements between views, 0 = one shared query); db_hw [batch, 2] int32 the views' (h, w);
 * query_h, query_w the query's.  The valid matches (matches0 > -1 and < n1) are compacted in
 * ascending index order inside the RANSAC kernel, (from, to) = (view, query) points.
 * Per view: counts [batch] the number of matches; mpts [batch, n0, 4] (x, y, X, Y) the compacted
 * correspondences (may be null); affine / inlier_mask [batch, n0] / n_inliers as above; status 0
 * = solved, 1 = fewer than 6 matches, 2 = no model; bbox [batch, 4] int32 (x0, y0, x1, y1) =
 * min / max of the view's corners (0,0), (w,0), (0,h), (w,h) through affine in double, each
 * truncated toward zero (astype(np.int32); a corner beyond int32 saturates here, where numpy
 * wraps -- no real view gets there).  Without an estimate (status 1 or 2) the box is the
 * reference's fallback [0, 0, query_h, query_w] -- its x1 is the height, as in the reference
 * (:98) -- and n_inliers 0; the reference would raise on status 2 (affine is None).
 * rank_mode 0 ranks a view by its number of matches (the reference: inliers.shape[0] of
 * OpenCV's N x 1 mask), 1 by its number of inliers; a view without an estimate ranks 0; the
 * first view in input order with the largest value wins (sorted(reverse=True) is stable):
 * best_view [1], best_bbox [4] int32.  n0 <= onepose_affine_partial_max_points(); workspace:
 * onepose_affine_partial_workspace_bytes(batch, n0).  All device pointers. */
int onepose_detect_stage(const int64_t* matches0, const int* counts0, const float* kpts0,
                         const float* kpts1, int64_t kpts1_bstride, const int* db_hw, int batch,
                         int n0, int n1, int query_h, int query_w, double threshold,
                         int max_iters, double confidence, int refine_iters, int rank_mode,
                         int* counts, float* mpts, double* affine, uint8_t* inlier_mask,
                         int* n_inliers, int* status, int* bbox, int* best_view, int* best_bbox,
                         void* workspace, size_t workspace_bytes, void* stream);
/* crop_img_by_bbox: image [h][w] uint8, bbox [4] int32 (x0, y0, x1, y1; a device pointer, e.g.
 * best_bbox), K [9] fp64 or null -> crop_u8 [crop_size][crop_size], crop_f32 = crop_u8 / 255
 * (may be null), K_crop [9] fp64 (null with K), crop_status [1] int32.  With bw = x1 - x0,
 * bh = y1 - y0 the reference's two warps (get_affine_transform with rot 0, read in closed form)
 * are T1 = [1 0 -x0; 0 1 -y0], an exact integer crop zero-filled outside the image, and T2 =
 * [s 0 tx; 0 s ty] with s = crop_size / bw in BOTH axes (data_utils.py:34 reads src_w only),
 * tx = crop_size/2 - s bw/2, ty = crop_size/2 - s bh/2: one bilinear warp of the zero-padded
 * bw x bh window in cv2.warpAffine's fixed-point arithmetic (1/1024 coordinate steps, 5
 * fractional bits, weights summing to 2^15), so the output is exact.  K_crop = T2 T1 K.
 * bw <= 0 or bh <= 0: crop_status 1, a zero image, K_crop = K (the reference would raise).
 * A box coordinate with |v| >= 2^15 (outside warpAffine's short maps; the integer walk would
 * leave int range): crop_status 2, a zero image, K_crop = K.  Else crop_status 0. */
int onepose_crop_resize(const uint8_t* image, int h, int w, const int* bbox, const double* K,
                        int crop_size, uint8_t* crop_u8, float* crop_f32, double* K_crop,
                        int* crop_status, void* stream);

/* ------------------------------------------------------------------------------------ *
 * NearestNeighbour 2D-2D matcher  --  replaces NearestNeighbour.forward
 *   (src/models/matchers/nn/nearest_neighbour.py: the einsum :42, find_nn :5-15 for rows and
 *    for columns :43-49, mutual_check :18-23), the matcher the reference's tracker runs per frame.
 * This family is versioned on its own, as the SuperGlue and detector families:
 * onepose_nn_version() returns 1; onepose_abi_version() was not bumped for it.
 *
 * sim[b][i][j] = sum_k desc0[b][k][i] desc1[b][k][j] is never stored: launch 1 is an fp32 MFMA
 * tile GEMM whose epilogue keeps, per 64 x 64 block, each row's and each column's (best value,
 * best index, second value); launch 2 merges those partials and applies find_nn's tests;
 * launch 3 (do_mutual_check only) is mutual_check.  Deterministic, no atomics.
 *
 * Kept from the reference:
 *  - a threshold that is not > 0 (the reference's falsy None / 0) or is NaN disables its test;
 *  - fp32 test arithmetic in the reference's order: dist = 2 * (1 - sim) is one subtraction and
 *    an exact doubling; ratio: dist_best <= float32(ratio ** 2) * dist_second, one multiply;
 *    distance: dist_best <= float32(distance ** 2); score (sim_best + 1) / 2, or 0 and -1;
 *  - only matches0 gets the mutual check: matches1 is the raw column result, mscores0 is NOT
 *    zeroed where the check clears matches0, and without the check matches0 is the raw row result;
 *  - descriptors are not normalised here: sim may leave [-1, 1] and dist may be negative;
 *  - the ratio test needs two candidates on both searched sides (topk(2) raises in the
 *    reference): n0 == 1 or n1 == 1 with a ratio test is ONEPOSE_ERR_INVALID;
 *  - the reference's conf key match_threshold is never read there and has no argument here.
 * Decided here (torch.topk promises no order on equal values): the best is the LOWEST index
 * among equal similarities, and the second value is the second element of the multiset, so a
 * duplicated best value is its own runner-up.  sim[i][j] is summed over k in one fixed order
 * wherever (i, j) lies in a tile, so bit-equal descriptor columns give bit-equal similarities.
 * NaN or infinite descriptors are outside the contract (a row that compares above nothing is
 * unmatched).
 *
 * desc0 [batch, d, n0], desc1 [batch, d, n1] in the reference's layout, fp32 (ONEPOSE_DT_F32)
 * or fp16 (ONEPOSE_DT_F16, converted as loaded: results are those of the fp32 call on the
 * upcast values, bit for bit); batch strides in elements, 0 = that side is shared by the batch.
 * 1 <= n0, n1 <= 16384, 1 <= d <= 1024 (any value), 1 <= batch <= 65535.
 * Outputs matches0 [batch, n0], matches1 [batch, n1] int64 (-1 = none), mscores0/1 fp32.
 * Checks, in this order, before anything is launched: null pointers (descriptors, outputs,
 * workspace); batch; n0 and n1; d; desc_dtype; negative strides; the ratio test's two
 * candidates -- all ONEPOSE_ERR_INVALID -- then the workspace size (ONEPOSE_ERR_WORKSPACE).
 * onepose_nn_match_workspace_bytes returns 0 for a refused shape.  The entry points never
 * allocate, free or synchronise and can be captured in a graph.  All device pointers.
 * onepose_nn_similarity_top2 is launch 1 alone (the partials stay in the workspace), for
 * measurement: the profile hook's kinds below are a closed list, so the launches of this
 * family are not bracketed by it.
 * ------------------------------------------------------------------------------------ */
int onepose_nn_version(void);
size_t onepose_nn_match_workspace_bytes(int batch, int n0, int n1);
int onepose_nn_match(const void* desc0, int64_t desc0_bstride, const void* desc1,
                     int64_t desc1_bstride, int desc_dtype, int batch, int d, int n0, int n1,
                     double ratio_threshold, double distance_threshold, int do_mutual_check,
                     int64_t* matches0, int64_t* matches1, float* mscores0, float* mscores1,
                     void* workspace, size_t workspace_bytes, void* stream);
int onepose_nn_similarity_top2(const void* desc0, int64_t desc0_bstride, const void* desc1,
                               int64_t desc1_bstride, int desc_dtype, int batch, int d, int n0,
                               int n1, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------ *
 * Tracker back end  --  bundle adjustment and triangulation, fp64
 *   onepose_ba_solve replaces BATracker.apply_ba's call of DeepLM's Solve
 *   (src/tracker/ba_tracker.py:358-441, the call at :401-407) with the cost function
 *   SnavelyReprojectionErrorV2 / AngleAxisRotatePoint (src/tracker/tracking_utils.py:91-169);
 *   onepose_triangulate replaces apply_triangulation (:267-273, cv2.triangulatePoints) together
 *   with track_ba's reprojection and depth filters (:556-571).
 * Versioned on its own: onepose_ba_version() returns 1; onepose_abi_version() was not bumped.
 *
 * What the reference pins: the cost function only.  residual[n] = f (R(aa) X + t).xy / (.).z +
 * (cx, cy) - (u, v) with X = points[ptIdx[n]], (aa, t) = cam_pose[camIdx[n]], (u, v, f, cx, cy) =
 * features[n]; the rotation takes the reference's two branches (theta^2 > 0: Rodrigues, else
 * X + aa x X), and at theta^2 == 0 the Jacobian is that branch's derivative, -[X]x.  For
 * 0 < theta^2 < 1e-4 the Jacobian's coefficients (1 - cos) / theta^2, (cos - sin / theta) /
 * theta^2 and (sin / theta - 2 (1 - cos) / theta^2) / theta^2 come from their series (the closed
 * forms cancel to nothing there and overflow at a subnormal theta^2); the residual does not
 * change.  DeepLM's
 * source is not in the reference tree and cv2 is not a dependency here, so the solver below is
 * this project's own (parity with DeepLM's iterates and with cv2's SVD is NOT verified); it is
 * restated in numpy float64 in tests/ba_oracle.py, which the GPU tests compare against.
 *
 * The solver: Ceres-style Levenberg-Marquardt, cost = 1/2 sum |residual|^2.  Per iteration:
 *   U_c = sum Jc^T Jc, V_p = sum Jp^T Jp, W_n = Jc^T Jp, g = J^T r at the current iterate;
 *   damping mu * clamp(diag, 1e-6, 1e32) with mu = 1 / radius is added to diag U and diag V;
 *   S = U - sum_p W V_p^-1 W^T over the active cameras, Cholesky, S dc = -g_c + W V^-1 g_p,
 *   dp = V^-1 (-g_p - W^T dc), where V_p^-1 is applied through its Cholesky factor (V = L L^T,
 *   Y = L^-1 W^T, W V^-1 W^T = Y^T Y) and never formed: an explicit inverse of a point seen by
 *   few cameras would cost S its accuracy;  candidate cost', model decrease md = -(J d).(r + J d / 2),
 *   rho = (cost - cost') / md;  accepted iff cost' is finite, md > 0 and rho > 1e-3.
 *   Accepted: radius = min(radius / max(1/3, 1 - (2 rho - 1)^3), 1e16), decrease factor = 2.
 *   Rejected, or a Cholesky pivot that is not > 0: radius /= factor, factor *= 2.
 * It stops after max_iters iterations or max_success accepted ones (the reference passes 5 and
 * 5; there are no convergence tolerances).  Only cameras and points with at least one
 * observation (the active ones) move; the others are never written.  On return the variables are
 * the last accepted iterate.  A non-finite initial cost gives status 1 with nothing moved.
 *
 * info [104] fp64, device: [0] status (0 ran, 1 non-finite initial cost, 2 the index does not
 * describe ptIdx / camIdx), [1] iterations, [2] accepted iterations, [3] initial cost, [4] final
 * cost, [5] final radius, [6..7] 0; then one row of 6 per iteration from [8]: cost, candidate
 * cost, model decrease, rho, the radius used, accepted (a failed Cholesky: NaN, NaN, NaN).
 *
 * The index (host): onepose_ba_build_index sorts the observations by camera and by point
 * (stable: ties stay in observation order) and lists the active cameras and points, into
 * onepose_ba_index_bytes(n_obs, n_cams, n_points) bytes of int32 words; it needs no GPU.  An id
 * outside [0, n_cams) / [0, n_points) is ONEPOSE_ERR_INVALID.  The caller uploads those bytes and
 * passes the two counts to the solve, whose first kernels check on the device that every id is in
 * range and that every CSR range holds, in observation order, exactly the observations of the
 * key it claims; on any mismatch the solve reports status 2 and moves nothing (nothing is
 * dereferenced through an unchecked index).
 *
 * points [n_points, 3], cam_pose [n_cams, 6], features [n_obs, 5] fp64; ptIdx, camIdx [n_obs]
 * int64.  1 <= n_obs <= 2^20, 1 <= n_cams, n_points <= 2^20, active cameras <=
 * onepose_ba_max_active_cameras() (24: the reference's windows are 10 and 20 keyframes plus the
 * current frame).  Checks of onepose_ba_solve, in this order, before anything is launched: null
 * pointers; shapes (sizes, active counts within 1..n); active cameras over the limit; max_iters
 * outside 1..16; max_success < 1; initial_radius not positive and finite -- all
 * ONEPOSE_ERR_INVALID -- then the workspace size (ONEPOSE_ERR_WORKSPACE).
 * onepose_ba_workspace_bytes returns 0 for a refused shape.
 *
 * onepose_ba_linearize is the first stage alone on the caller's arrays (no index): residuals
 * [n_obs, 2], Jc [n_obs, 2, 6], Jp [n_obs, 2, 3], cost [1].  An observation whose ids are out of
 * range gets NaN rows (and the cost is NaN); nothing is read through them.
 *
 * onepose_triangulate: P1, P2 [3, 4] projection matrices (K inv(Tcw)[:3]), pts1, pts2 [n, 2]
 * pixels -> X [n, 3], err1, err2 [n] (reprojection error in each view), z [n] (= X[:, 2]), keep
 * [n] uint8 = err1 <= rep_thr && err2 <= rep_thr && z <= z_max (the reference removes > 20 and
 * > 0.15); a pair with w == 0 or any non-finite result is not kept.  One thread per pair: the
 * 4 x 4 DLT matrix A, the eigenvector of A^T A's smallest eigenvalue by cyclic Jacobi (the
 * reference's own _triangulatePy, :243-265, also works on A^T A), dehomogenised.
 *
 * No entry point allocates, frees or synchronises; all can be captured in a graph.  No
 * floating-point atomics and a fixed order in every sum: results are bit-identical from run to
 * run and on any stream.  All pointers are device pointers except those of
 * onepose_ba_build_index, which are host pointers.  The profile hook's kinds are a closed list,
 * so the launches of this family are not bracketed by it.
 * ------------------------------------------------------------------------------------ */
int onepose_ba_version(void);
int onepose_ba_max_active_cameras(void);
size_t onepose_ba_index_bytes(int64_t n_obs, int n_cams, int n_points);
int onepose_ba_build_index(const int64_t* ptIdx, const int64_t* camIdx, int64_t n_obs, int n_cams,
                           int n_points, void* index, size_t index_bytes, int* n_active_cams,
                           int* n_active_points);
size_t onepose_ba_workspace_bytes(int64_t n_obs, int n_active_cams, int n_active_points);
int onepose_ba_solve(double* points, double* cam_pose, const double* features,
                     const int64_t* ptIdx, const int64_t* camIdx, const void* index,
                     int64_t n_obs, int n_cams, int n_points, int n_active_cams,
                     int n_active_points, int max_iters, int max_success, double initial_radius,
                     double* info, void* workspace, size_t workspace_bytes, void* stream);
int onepose_ba_linearize(const double* points, const double* cam_pose, const double* features,
                         const int64_t* ptIdx, const int64_t* camIdx, int64_t n_obs, int n_cams,
                         int n_points, double* residuals, double* Jc, double* Jp, double* cost,
                         void* stream);
int onepose_triangulate(const double* P1, const double* P2, const double* pts1,
                        const double* pts2, int n, double rep_thr, double z_max, double* X,
                        double* err1, double* err2, double* z, uint8_t* keep, void* stream);

/* ------------------------------------------------------------------------------------ *
 * Tracker front end  --  pyramidal Lucas-Kanade optical flow
 *   onepose_lk_build_pyramid + onepose_lk_track replace cv2.calcOpticalFlowPyrLK as
 *   BATracker.kpt_flow_track calls it (src/tracker/ba_tracker.py:113-126: 8-bit single-channel
 *   images, winSize 15 x 15, maxLevel 2, criteria (EPS | COUNT, 10, 0.03), no flags).
 * Versioned on its own: onepose_lk_version() returns 1; onepose_abi_version() was not bumped.
 * Not produced: cv2's err output (the reference discards it).  Not supported:
 * OPTFLOW_USE_INITIAL_FLOW, OPTFLOW_LK_GET_MIN_EIGENVALS, multi-channel or non-8-bit images,
 * non-square windows.
 *
 * No OpenCV source or binary is at hand, so parity with cv2 itself is NOT verified; what is
 * assumed about OpenCV 4.4 is listed in DESIGN.md.  The contract below is what the kernels
 * compute; tests/lk_oracle.py restates it in numpy and the GPU tests ask for equal bits.
 *
 * Limits, checked on the host before any launch (a _bytes / _levels query returns 0 for an
 * unsupported shape, the other entry points ONEPOSE_ERR_INVALID):  win odd, 3 <= win <= 31;
 * 0 <= max_level <= 5;  win < h, w <= 8192;  1 <= batch <= 65535;  0 <= max_points <= 2^24
 * (max_points == 0 is a no-op that returns 0);  max_count is clamped to [0, 100] and epsilon to
 * [0, 10] and then squared (in double, rounded to float once), as cv2 does;  NaN epsilon or
 * min_eig_threshold is refused;  a batch stride is 0 (shared) or at least one item.  counts is a
 * device array, so the host cannot see it: the kernel clamps counts[b] to [0, max_points].
 *
 * The pyramid blob (onepose_lk_pyramid_bytes per image, a multiple of 256): per level, the image
 * uint8 [lh, lw] and then the derivative int16 [lh, lw, 2] (dx, dy interleaved), each at a
 * 256-byte-aligned offset that onepose_lk_pyramid_layout (a host function) reports, so a level
 * is a plain view of the blob.  No border is stored.  The derivative space is reserved but not
 * written with with_deriv == 0 (the next image of a pair needs none).  Two launches per call:
 * level 0 with its derivative and level 1 from the image; then levels >= 1 by one workgroup per
 * image (skipped when nothing is left for it).  Images of more than 1024 x 1024 pixels get one
 * grid launch per level >= 1 in place of that workgroup.
 *
 * pyrDown: [1 4 6 4 1] horizontally then vertically in integers, output ((h+1)/2, (w+1)/2),
 *   output (y, x) centred on (2y, 2x), source indices reflected (BORDER_REFLECT_101),
 *   (sum + 128) >> 8.
 * Levels: level l + 1 is built only while l < max_level and its width and height both exceed
 *   win; onepose_lk_levels returns the number built (>= 1).
 * Scharr: rows reflected-101 inside the level, t0 = (up + down) * 3 + cur * 10, t1 = down - up;
 *   columns reflected-101, dx = t0[x+1] - t0[x-1], dy = (t1[x+1] + t1[x-1]) * 3 + t1[x] * 10.
 * Reads outside a level (up to win pixels): image reflected-101, derivative zero.
 * Per point, per level l from the top down to 0, all floats fp32, every step a separate
 * operation in this order (no fused multiply-add), sqrt and / correctly rounded:
 *   prev = pts * (1 / (1 << l));  next = prev at the top level, else next = next * 2;
 *   half = (win - 1) * 0.5;  p = prev - half;  ip = floor(p);
 *   OUT(ip): ip.x < -win || ip.x >= cols || ip.y < -win || ip.y >= rows, decided by float
 *     comparisons on floor(p) before any conversion to integer (NaN is OUT);
 *   if OUT(ip): status = 0 if l == 0; go to the next level;
 *   a = p.x - ip.x, b = p.y - ip.y;  iw00 = rint((1-a)(1-b) 2^14), iw01 = rint(a (1-b) 2^14),
 *   iw10 = rint((1-a) b 2^14), iw11 = 2^14 - iw00 - iw01 - iw10 (round half to even);
 *   descale(v, n) = (v + (1 << (n-1))) >> n;  over the win x win window at ip:
 *   I = descale(4-tap image sum, 9);  Ix, Iy = descale(4-tap derivative sum, 14);
 *   A11, A12, A22 = the exact integer sums of Ix^2, Ix Iy, Iy^2, each converted to float once
 *     (round to nearest even) and multiplied by 2^-20;
 *   D = A11 A22 - A12 A12;
 *   minEig = (A22 + A11 - sqrt((A11 - A22)(A11 - A22) + 4 A12 A12)) / (2 win^2);
 *   if minEig < min_eig_threshold || D < FLT_EPSILON: status = 0 if l == 0; next level;
 *   Dinv = 1 / D;  n = next - half;  prevDelta = 0;  up to max_count times (j = 0, 1, ...):
 *     if OUT(floor(n)): status = 0 if l == 0; break;
 *     weights from n;  diff = descale(4-tap sum of the next image, 9) - I;
 *     b1, b2 = the exact integer sums of diff Ix, diff Iy, converted once, times 2^-20;
 *     delta = ((A12 b2 - A22 b1) Dinv, (A12 b1 - A11 b2) Dinv);  n += delta;  next = n + half;
 *     if delta.x delta.x + delta.y delta.y <= epsilon^2: break;
 *     if j > 0 && |delta.x + prevDelta.x| < 0.01 && |delta.y + prevDelta.y| < 0.01:
 *       next -= delta * 0.5; break;
 *     prevDelta = delta.
 *   status starts at 1; next_pts = next after level 0.
 * The sums are integers reduced across the wave, so the result does not depend on the lane
 * mapping or the summation order and is bit-identical from run to run (cv2 accumulates the same
 * terms in float, in an order that depends on its SIMD path: a stated difference of at most
 * rounding).
 * A point that is NaN, infinite or of magnitude >= 2^30 gets status 0 and next_pts = prev_pts,
 * bit for bit, before anything is computed from it (the rule above gives the same result for
 * the finite ones; this spares them the arithmetic).
 *
 * onepose_lk_track: one wave per point, four points per 256-thread workgroup, one launch.
 * prev_pyr (prev_pyr_bstride BYTES per item, 0 = shared) needs its derivatives; next_pyr
 * [batch x pyramid_bytes];  prev_pts [.., max_points, 2] fp32 (prev_pts_bstride FLOATS per item,
 * 0 = shared);  next_pts [batch, max_points, 2], status [batch, max_points]: rows from
 * counts[b] on are not written.  No entry point allocates, frees or synchronises; all can be
 * captured in a graph.  All pointers are device pointers except the four outputs of
 * onepose_lk_pyramid_layout.
 * ------------------------------------------------------------------------------------ */
int onepose_lk_version(void);
int onepose_lk_levels(int h, int w, int win, int max_level);
size_t onepose_lk_pyramid_bytes(int h, int w, int win, int max_level);
int onepose_lk_pyramid_layout(int h, int w, int win, int max_level, int level, int* lh, int* lw,
                              int64_t* image_offset, int64_t* deriv_offset);
int onepose_lk_build_pyramid(const uint8_t* image, int64_t image_bstride, int batch, int h, int w,
                             int win, int max_level, int with_deriv, void* pyramids,
                             void* stream);
int onepose_lk_track(const void* prev_pyr, int64_t prev_pyr_bstride, const void* next_pyr,
                     const float* prev_pts, int64_t prev_pts_bstride, const int* counts, int batch,
                     int max_points, int h, int w, int win, int max_level, int max_count,
                     float epsilon, float min_eig_threshold, float* next_pts, uint8_t* status,
                     void* stream);

/* ------------------------------------------------------------------------------------ *
 * Object builder  --  SfM filter, merge and descriptor lifting
 *   The reference's postprocess stage (run.py:196-249): filter_points.filter_3d and
 *   filter_points.merge (src/sfm/postprocess/filter_points.py:8-117) and
 *   feature_process.get_kpt_ann's gather and averaging (feature_process.py:59-188, 297-305),
 *   plus data_utils.build_features3d_leaves' gather (src/utils/data_utils.py:163-205).
 * Versioned on its own: onepose_objbuild_version() returns 1; onepose_abi_version() was not
 * bumped.  Not here: score means (numpy sums a [k, 1] column pairwise; they stay on the host),
 * the leaf permutation (numpy's RNG; the host supplies the indices), anno_2d.json.
 *
 * Every floating-point step below is one IEEE operation, rounded to nearest even, in the order
 * written; a*b + c is never fused; sqrt and / are correctly rounded.  No floating-point atomics
 * and a fixed order in every sum: results are bit-identical from run to run.  Merge and lifting
 * reproduce the reference bit for bit; the box test's dot product is this project's own order
 * (torch.matmul's differs in the last bits), so it is pinned to the reference only for points
 * that keep a margin from every face.
 *
 * All pointers are device pointers.  No entry point allocates, frees or synchronises.  Checks
 * on the host (null pointers, sizes, flags) return ONEPOSE_ERR_INVALID before anything is
 * launched, and nothing is written.  What only the device can see is reported in a device
 * `info` array, and the call then writes nothing but what is said below.
 *
 * onepose_filter_points: stable compaction.  xyz [n, 3] fp64 in ascending point-id order,
 *   track_len [n] int32 (NULL: no track filter), corners [8, 3] fp64 (NULL: no box filter),
 *   1 <= n <= 2^24.  Point i is kept iff track_len[i] >= min_track and it passes the box test:
 *     c = float32(corners), p = float32(xyz[i]);  q = p - c[4];
 *     for v in (c[5] - c[4], c[0] - c[4], c[7] - c[4]):
 *       m = (q0 v0 + q1 v1) + q2 v2;  vv = (v0 v0 + v1 v1) + v2 v2;  pass iff 0 < m and m < vv
 *   all in fp32, both comparisons strict, so a point on a face and a NaN coordinate fail.
 *   xyz_out [n, 3] fp32 = float32(xyz[i]) and index_out [n] int32 = i for the kept points, in
 *   input order; count [1] int32.  Rows from count on are not written.  One workgroup walks the
 *   points 1024 at a time.
 *
 * onepose_radius_neighbours: xyz [n, 3] of xyz_dtype (ONEPOSE_OBJ_F32 / _F64), 1 <= n <= 65536,
 *   thr positive and finite.  i is a neighbour of j iff i == j or sqrt(s) < thr with
 *     dx = double(x_i) - double(x_j), dy, dz alike;  s = (dx dx + dy dy) + dz dz
 *   (scipy's pdist on the widened values; squareform's diagonal is 0, hence i == j).  Output: a
 *   CSR, row_start [n + 1] int32 and cols [cols_capacity] int32, row j holding its neighbours
 *   ascending.  Three launches: a count per row (one wave per row), a scan, and the same walk
 *   again placing each lane by a ballot prefix; the n x n matrix is never written.
 *   info [2] int64: [0] the total number of pairs, [1] 0 written, 1 the total exceeds
 *   cols_capacity, 2 it exceeds 2^31 - 1.  With [1] != 0 nothing is written to cols and
 *   row_start is not to be used; cols_capacity == 0 (cols may be NULL) is the size query.
 *
 * onepose_merge_greedy: the greedy pass over that CSR, on the same xyz.  For j = 0 .. n - 1: if
 *   any neighbour of j is already recorded, skip j; otherwise the neighbours of j become the next
 *   cluster and are recorded.  A skipped point that no later cluster picks up is dropped (for a
 *   chain a-b-c seeded at a the cluster is {a, b} and c is lost), as in the reference.
 *   cluster_of [n] int32 (-1: dropped);  member_start [n + 1] int32 and members [n] int32, a CSR
 *   of each cluster's points ascending;  mean [n, 3] fp64, of which the first info[0] rows are
 *   written:  s = x[m0]; s = s + x[m1]; ... in the member order and in the dtype of xyz, then
 *   s / count in that dtype, then widened.  info [2] int32: [0] the cluster count, [1] 0, or 1
 *   when row_start / cols is not a CSR over n points (an entry outside [0, n), an empty row, more
 *   members than points); the other outputs are then unspecified, and nothing was read or
 *   written through the bad entry.  The pass is sequential in j by definition: one wave, at most
 *   n row visits (worst case: no row is its own only neighbour); a run of consecutive rows that
 *   are each their own only neighbour becomes a run of clusters in one step.
 *
 * onepose_lift_descriptors: the 3D descriptor lifting.  bank: bank_numel fp32, holding image
 *   block b as [dim, block_cols[b]] (as the extractor emits it) from element block_offset[b]
 *   (int64); observation o is column obs_feat[o] of block obs_block[o] (both int32), in collect
 *   order; seg_len [n3] int32 is the reference's idxs (observations per 3D point).
 *   1 <= dim <= 1024, 1 <= n3 <= n_obs <= 2^28, 1 <= n_blocks <= 2^20.
 *     collected [dim, n_obs] fp64 = double(bank value);
 *     mean64 [dim, n3] fp64:  s = first; s = s + next; ... over the segment in observation order,
 *       then s / double(count);   mean32 [dim, n3] fp32 = float32(mean64);
 *     seg_start [n3 + 1] int32: the segments' first observations.
 *   The sum is sequential at every dim.  That is the reference's mean_descriptors bit for bit
 *   for dim >= 2 (np.mean(axis=0) on a [k, dim] block adds row by row).  At dim == 1 the block is
 *   one contiguous run and numpy sums it pairwise, so the reference -- and this package's
 *   device=None path, which takes the reference's route -- may differ from the device there.
 *   info [2] int32: [0] 0, or 1 a segment of length < 1, 2 the lengths do not add up to n_obs,
 *   3 a block outside the bank, 4 an observation outside its block; [1] the smallest offending
 *   index.  With [0] != 0 none of collected, mean64, mean32 is written (a block that no
 *   observation uses is fine).  One thread per (3D point, channel).
 *
 * onepose_gather_leaves: out [dim, n_cols] fp32, column i = float32(collected[:, cols[i]]);
 *   cols [n_cols] int64, where cols[i] == n_obs is the dustbin, a column of ones; any other
 *   value outside [0, n_obs) gives a column of NaN and nothing is read through it.
 * ------------------------------------------------------------------------------------ */
#define ONEPOSE_OBJ_F32 0
#define ONEPOSE_OBJ_F64 1
int onepose_objbuild_version(void);
int onepose_filter_points(const double* xyz, const int* track_len, int n, int min_track,
                          const double* corners, float* xyz_out, int* index_out, int* count,
                          void* stream);
int onepose_radius_neighbours(const void* xyz, int xyz_dtype, int n, double thr, int* row_start,
                              int* cols, int64_t cols_capacity, int64_t* info, void* stream);
int onepose_merge_greedy(const void* xyz, int xyz_dtype, int n, const int* row_start,
                         const int* cols, int* cluster_of, int* member_start, int* members,
                         double* mean, int* info, void* stream);
int onepose_lift_descriptors(const float* bank, int64_t bank_numel, const int64_t* block_offset,
                             const int* block_cols, int n_blocks, const int* obs_block,
                             const int* obs_feat, int n_obs, const int* seg_len, int n3, int dim,
                             int* seg_start, double* collected, double* mean64, float* mean32,
                             int* info, void* stream);
int onepose_gather_leaves(const double* collected, int n_obs, int dim, const int64_t* cols,
                          int n_cols, float* out, void* stream);

/* ------------------------------------------------------------------------------------ *
 * Sparse reconstruction  --  feature tracks and multi-view triangulation
 *   The part of the reference's sfm_core (run.py:140-193) that follows matching: the tracks that
 *   COLMAP forms from the imported matches, and the points its point_triangulator computes from
 *   them with the poses held fixed (src/sfm/triangulation.py:122-148).
 * Versioned on its own: onepose_sfm_version() returns 1; onepose_abi_version() was not bumped.
 *
 * No COLMAP source or binary is at hand, so the triangulator below is this project's own:
 * parity with COLMAP's point_triangulator is NOT verified and is not claimed.  The defaults the
 * Python layer passes (max_reproj 4 px, min_angle 1.5 degrees) follow COLMAP's documented mapper
 * defaults in name only.  Not here: geometric verification, RANSAC over the observations, bundle
 * adjustment, point colours.  tests/sfm_oracle.py restates both entry points in plain loops.
 *
 * All pointers are device pointers.  No entry point allocates, frees or synchronises; both can
 * be captured in a graph, and the launch sequence of a call depends on its host arguments only.
 * No floating-point atomics, and every sum over a track's observations is taken in ascending
 * position: results are bit-identical from run to run.  a*b + c is never fused.  Host checks
 * (null pointers, sizes, NaN thresholds) return ONEPOSE_ERR_INVALID before anything is launched.
 *
 * onepose_track_components: connected components of the graph whose nodes are the features
 *   (global feature id = the image's feature offset + the keypoint index) and whose edges
 *   [n_edges, 2] int32 are the matches.  parent [n_nodes] int32: on return the label of a node is
 *   the smallest id of its component.  That result is unique, so the integer atomicMin below
 *   leaves nothing to scheduling.  1 <= n_nodes <= 2^30, 0 <= n_edges <= 2^30 (edges may be NULL
 *   at 0), 0 <= rounds <= 64.  Launches: one that sets parent[i] = i when init != 0 and zeroes
 *   status; then per round
 *     compress: every node walks to its root (parent[r] == r) and stores it.  parent[x] <= x
 *       holds throughout and a parent only ever decreases, so a concurrent reader sees a node of
 *       the same component; a root is never written, so every walk ends at a true root;
 *     hook: per edge with roots ru != rv, atomicMin(&parent[max(ru, rv)], min(ru, rv)).  The
 *       launch returns at once when the previous round joined nothing;
 *   then a final compress and a check.  status [4] int32: [0] the edges whose ends still carry
 *   different labels (0: converged), [1] the rounds that joined something, [2] the edges with an
 *   end outside [0, n_nodes): they are ignored and nothing is read through them, [3] internal.
 *   With init == 0 the call continues from parent as an earlier call left it, so a caller loops
 *   while status[0] != 0 and correctness never rests on `rounds`; a parent value outside [0, x]
 *   (an array no first call wrote) ends a walk, and nothing is read through it.
 *
 * onepose_tracks_triangulate: Rt [n_images, 3, 4] (x_cam = R X + t) and K4 [n_images, 4] = (fx,
 *   fy, cx, cy), fp64; the tracks as a CSR, track_start [n_tracks + 1] int32 over obs_image
 *   [n_obs] int32 (an index into Rt / K4) and obs_xy [n_obs, 2] fp64 pixels (the Python layer
 *   adds 0.5 to the extractor's keypoints, as the reference's import_features does).
 *   1 <= n_tracks <= 2^24, 1 <= n_obs <= 2^28.  Two launches: the check, then one wave per track.
 *   The check (one workgroup) runs before anything is read through the CSR: status [2] int32,
 *   [0] = 0, or 1 when track_start is not 0 = s[0] <= s[1] <= ... <= s[n_tracks] = n_obs, or 2
 *   when an image id lies outside [0, n_images); [1] the smallest offending index.  With
 *   status[0] != 0 no output is written.
 *   Per track, with S = all its observations (positions 0 .. len - 1):
 *   1 DLT: an observation contributes the rows xn Rt[2] - Rt[0] and yn Rt[2] - Rt[1], xn = (u -
 *     cx) / fx, yn = (v - cy) / fy.  M = A^T A, each entry summed over S as m = m + (a_i a_j +
 *     b_i b_j); the eigenvector of its smallest eigenvalue by cyclic Jacobi, exactly as
 *     onepose_triangulate takes it; X = h[0:3] / h[3].
 *   2 Score: p = Rt X, residual = (fx p0 / p2 + cx - u, fy p1 / p2 + cy - v), e = its norm; an
 *     observation is an inlier iff p2 > 0 and e <= max_reproj.  If any observation of S fails,
 *     the worst leaves S (the largest e, p2 <= 0 counting as +inf, ties to the lowest position)
 *     and step 1 runs again; fewer than 2 left: reason 1.
 *   3 Duplicates: of several observations of S in one image the one with the smallest e stays
 *     (ties to the lowest position); fewer than 2 left: reason 1.
 *   4 Refine: at most 5 Gauss-Newton steps on cost = sum over S of |residual|^2.  H = sum J^T J,
 *     g = sum J^T r with J = d residual / dX; H = L L^T, H d = -g; X + d is taken iff its cost is
 *     strictly smaller.  The first rejected step or pivot that is not > 0 ends the refinement.
 *   5 Final check: e at the refined X; observations that now fail leave S (no new solve); fewer
 *     than 2 left: reason 1.  With unit rays from X to the camera centres -R^T t, the largest
 *     angle between two rays of S is acos(clamp(smallest dot product)); below min_angle_deg:
 *     reason 2.
 *   A track of length < 2 or > onepose_sfm_max_track() (256): reason 3, nothing read.  A
 *   non-finite X after a solve, or a NaN error or dot product: reason 4.
 *   Outputs: reason [n_tracks] int32 (0: kept); xyz [n_tracks, 3]; err [n_tracks], the mean of e
 *   over the final S, summed in ascending position; n_kept [n_tracks] int32 = |S|; obs_keep
 *   [n_obs] uint8, 1 for the final S.  A track with reason != 0 gets NaN, NaN, 0 and zeros.
 *   Mapping: lanes over the observations for the per-observation terms, which are staged in LDS
 *   (20 KB per wave; no per-thread array is indexed at run time); ten lanes each sum one unique
 *   entry of A^T A (then of H, g and the cost) serially; every lane then holds the sums and runs
 *   the 4 x 4 Jacobi and the 3 x 3 Cholesky itself.
 * ------------------------------------------------------------------------------------ */
int onepose_sfm_version(void);
int onepose_sfm_max_track(void);
int onepose_track_components(const int* edges, int n_edges, int n_nodes, int rounds, int init,
                             int* parent, int* status, void* stream);
int onepose_tracks_triangulate(const double* Rt, const double* K4, int n_images,
                               const int* track_start, const int* obs_image, const double* obs_xy,
                               int n_tracks, int n_obs, double max_reproj, double min_angle_deg,
                               double* xyz, double* err, int* reason, int* n_kept,
                               uint8_t* obs_keep, int* status, void* stream);

/* ------------------------------------------------------------------------------------ *
 * Measurement hook (bench.py's roofline). While enabled, every launch whose kernel kind
 * is in `kind_mask` (bit k = kind k, names from onepose_profile_kind_name) is bracketed by
 * two HIP events recorded on the launch's own stream.  Host-side state, not for use during
 * graph capture.  _end synchronises and returns, per bracketed launch, its kind and the
 * elapsed milliseconds between its two events.
 * ------------------------------------------------------------------------------------ */
int onepose_profile_begin(uint64_t kind_mask, int capacity);
/* Device-stamp variant, usable inside captured HIP graphs (event brackets are not).  While
 * enabled, each launch of a masked kind that supports stamps (the token GEMMs: kv/q/mlp1/
 * mlp2/final/score) is timed by its own workgroups on the device's constant-rate clock
 * (s_memrealtime): first workgroup start to last workgroup end; the last workgroup adds the
 * duration to a per-kind total and re-arms the slot, so graph replays and repeated launches
 * all accumulate.  Each launch (or captured graph node) draws its own accumulator from a
 * per-kind pool of 256, so launches of one kind may run concurrently.  A graph
 * captured while enabled carries the accumulator address and keeps timing when replayed;
 * calling _begin_device again re-zeroes the accumulators (same addresses).
 * _end_device synchronises the device and returns, per kind k < n_kinds, the number of
 * launches timed and their total milliseconds. */
int onepose_profile_begin_device(uint64_t kind_mask);
int onepose_profile_end_device(int64_t* launches, double* total_ms, int n_kinds);
int onepose_profile_end(int* kinds, float* ms, int capacity, int* count);
const char* onepose_profile_kind_name(int kind);

#ifdef __cplusplus
}
#endif

/* Families added after ABI 9 keep their declarations and contract in a header of their own. */
#include "onepose_two_view.h"   /* two-view verification: batched F-matrix RANSAC */
#include "onepose_superglue_counts.h"   /* SuperGlue batches of unequal counts and image sizes */
#include "onepose_global_ba.h"   /* global bundle adjustment: Schur-PCG Levenberg-Marquardt */
#include "onepose_match_counts.h"   /* the 2D-3D matcher with per-sample keypoint counts */

#endif /* ONEPOSE_HIP_H */
