/* lcr_hip.h — C ABI of liblcr_hip.so: the MI355X (gfx950) implementation of LCR-Net's per-scan hot path.
 *
 * Drop-in boundary.  The reference binds its native ops with pybind11 as module `utils.ext`
 * (utils/extensions/pybind.cpp:7-24) and calls them from experiments/lcrnet/modules/ops/{grid_subsample,radius_search}.py.  This header is
 * what a foreign-function binding (ctypes / cffi / cgo) would bind instead; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in `_host`; all memory is caller-owned;
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous and stream-ordered, does not
 *     synchronise the host and does not allocate — with these stated exceptions:
 *       lcr_precompute_batch[_rows] ends with ONE synchronisation of `stream` (it returns the per-stage
 *       lengths of the batch on the host) and owns a small per-process pool of side streams, events and
 *       pinned staging words, created on first use and kept until process exit;
 *       lcr_ktimer_read synchronises on the events it logged (measurement harness only);
 *       the opt-in stream-K GEMM keeps one library-owned device scratch buffer per (device, stream), allocated on first use;
 *   - all other scratch memory comes from the caller: ask `*_ws_bytes`, pass `ws`/`ws_bytes`;
 *   - stacked ("stack mode") clouds: points f32[N,3] row-major, lengths i64[B] (reference layout,
 *     utils/extensions/cpu/grid_subsampling/grid_subsampling.cpp:20-30);
 *   - return value: 0 ok, -1 bad argument, -2 workspace/output too small, -3 HIP launch error
 *     (text via lcr_last_error()).  Data-dependent conditions are reported through the `status` words;
 *   - every nonzero code comes with a text of the form `<called entry>: ...` — the name is that of the entry point the caller called,
 *     also where a legacy entry forwards to its `_ex` / `_rows` twin or one entry sizes or builds something through another's body.
 *     One exception: the native drivers (lcr_encoder_forward[_ex], lcr_roformer_forward, lcr_precompute_batch[_rows[_ex]],
 *     lcr_netvlad_forward / _train_forward / _backward) check their own arguments in their own name but run their operators through the
 *     public entries of this header, so what an operator refuses — a launch error, or a weight table whose widths are outside the
 *     operator's domain — carries the OPERATOR's name (`lcr_kpconv_aggregate_mask: C must be ...` out of lcr_encoder_forward_ex).
 *     The text is per host thread, and a successful call does not clear it: read lcr_last_error() only after a nonzero code.
 *
 * Shape domain (what the kernels are built for = every shape of the shipped configuration, experiments/lcrnet/config_model.py:33-43 with
 * best-model-mixed.tar, and of BASELINE.json's configs; a call outside it returns LCR_EARG with a message, it never computes something else):
 *   - clouds per call (B): 1..64 for the support grids / radius searches / lcr_precompute_batch (GRID_MAX_B); batches of more scans are
 *     split by the caller (lcr-net_amd/pipeline.py feeds 8 per call, PairPipeline at most 32 pairs = 64 clouds); 1..128 for
 *     lcr_augment_clouds (a loop-detection training batch is 6 x 13 = 78 clouds; the training head's own cap is 128 segments);
 *   - neighbour columns per row (`limit`, H): 1..128 for the KPConv aggregation / C_in = 1 KPConv / max-pool (KP_HMAX; the reference's
 *     calibrated limits are 64..80); the radius search itself accepts any limit >= 1 (balls with more than 512 hits take an exact
 *     storage-free path) and limit <= 0 = count-only;
 *   - KPConv feature width (C_in = C_out = mid channels of a ResidualBlock): 32, 64, 128 or 256 (init_dim 64 -> 32..256), 15 kernel points;
 *     C_in = 1 (encoder1_1) has its own fused kernel with any C_out <= 256;
 *   - GroupNorm: channels % 4 == 0 and % groups == 0 (32 groups in the reference); segment tables (per scan or per pair) of S <= 256
 *     segments with S * groups <= 2048;
 *   - lcr_encoder_forward: exactly the KPEncoder of backbone4.py:11-89 — 4 stages, ConvBlock + 10 ResidualBlocks in that order, any
 *     init_dim whose block widths fall in the KPConv domain above.  Other depths run block by block through the same building-block
 *     entries (lcr-net_amd/modules/kpconv/modules.py does that when `native_encoder.eligible` says no);
 *   - GEMMs: any M; N, K >= 1 (K % 4 == 0 for the vectorised forms, else the generic tile); the split-bf16 form needs K >= 288, K % 32 == 0, N >= 64;
 *   - attention: head dim 32 (d_model 128 / 4 heads in the reference), <= 64 stacked problems per segmented call; dense form any key count,
 *     top-k form <= 4096 keys per cloud (the scores of a row live in LDS: 70 KB of the 160 KB of a gfx950 CU — this library targets gfx950 only);
 *   - retrieval: descriptor width % 4 == 0 (256 in the reference), k <= 128 (50 in the reference), any corpus size that fits HBM;
 *   - pose tail: <= 4000 coarse nodes per cloud, patches of <= 128 points (+ dustbin: 129 x 129 transport problems; point_limit 128 in the
 *     reference), 3 x 3 weighted Procrustes.
 */
#ifndef LCR_HIP_H
#define LCR_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LCR_OK 0
#define LCR_EARG (-1)
#define LCR_ESPACE (-2)
#define LCR_EHIP (-3)

/* bits of the device-side status word written by data-dependent stages */
#define LCR_STATUS_KEY_OVERFLOW 1u   /* voxel key needs more than 64 bits together with the cloud id */
#define LCR_STATUS_LEN_MISMATCH 2u
#define LCR_GN_REPLICAS 8  /* copies of every GroupNorm statistics table (see lcr_gemm_f32) */   /* sum(lengths) exceeds the capacity passed by the host */

const char* lcr_last_error(void);
/* Opt-in launch timing for measurement harnesses (bench.py's roofline leg): while enabled, lcr_gemm_f32 (kind 0, meta = M,N,K)
 * and lcr_kpconv_aggregate (kind 1, meta = M,Ns,H,C,index bytes) bracket their launch with HIP events on the launch stream —
 * also when they are called from lcr_encoder_forward.  lcr_ktimer_enable(1) clears the log; lcr_ktimer_read synchronises on
 * the logged events and returns the number of records of `kind`. */
void lcr_ktimer_enable(int on);
void lcr_ktimer_sample(int every);   /* time every n-th instrumented launch of a kind only (default 1 = all) */
void lcr_ktimer_kinds(unsigned mask); /* time only the kinds whose bit is set (gemm 0, aggregate 1, radius 2, attention 3, fused 4, sinkhorn 5; default all) */
int lcr_ktimer_read(int kind, int max_records, double* seconds, int64_t* meta);
/* same, plus the kernel's own begin-to-end duration (what a profiler reports; < 0 where a launch site does not record it) */
int lcr_ktimer_read2(int kind, int max_records, double* seconds, double* seconds_kernel, int64_t* meta);
/* One wavefront spinning for `microseconds` on `stream`.  The runtime deals streams to 4 hardware queues; two busy
 * streams on one queue serialise each other.  A short kernel on stream B behind a spin on stream A tells whether A and B share
 * a queue (lcr-net_amd/pipeline.py picks its streams on distinct queues this way).  Test / tuning hooks live in lcr_hip_debug.h. */
int lcr_stream_spin(int microseconds, void* stream);
int lcr_version(void);

/* ------------------------------------------------------------------------------------------------
 * a-1  grid subsampling — replaces utils.ext.grid_subsampling
 *      (utils/extensions/cpu/grid_subsampling/grid_subsampling.cpp:5-62 → grid_subsampling_cpu.cpp:3-75).
 * Barycentre of every occupied voxel, per cloud; fp32 sums in INPUT order; output in libstdc++
 * std::unordered_map iteration order (bit-exact with the reference).
 *   xyz      f32[n_cap,3]   stacked input clouds (first sum(len) rows are used)
 *   len      i64[B]
 *   out_xyz  f32[n_cap,3]   first sum(out_len) rows are written
 *   out_len  i64[B]
 *   status   u32[1]         OR-ed LCR_STATUS_* bits (must be zeroed by the caller once)
 * ------------------------------------------------------------------------------------------------ */
int lcr_grid_subsample_ws_bytes(int64_t n_cap, int B, size_t* bytes);
int lcr_grid_subsample(const float* xyz, const int64_t* len, int B, int64_t n_cap, float voxel,
                       float* out_xyz, int64_t* out_len, uint32_t* status,
                       void* ws, size_t ws_bytes, void* stream);
/* Same, with a host-side promise that (voxel key bits + cloud id bits) <= key_bits_hint (0 = unknown, 64-bit safe):
 * bounds the number of radix passes launched.  A violated promise sets LCR_STATUS_KEY_OVERFLOW; retry with 0. */
int lcr_grid_subsample_ex(const float* xyz, const int64_t* len, int B, int64_t n_cap, float voxel, int key_bits_hint,
                          float* out_xyz, int64_t* out_len, uint32_t* status,
                          void* ws, size_t ws_bytes, void* stream);
/* Same on rows of `row_floats` (3 .. 64) floats whose first three are x, y, z — a KITTI velodyne scan f32[N,4] (x, y, z, intensity:
 * data/Kitti/downsample_pcd.py:21; dataset_overlap_online.py:245 slices [:, :3] on the host) is consumed as it lies in memory; the
 * output is f32[M,3]. */
int lcr_grid_subsample_rows(const float* xyz, int row_floats, const int64_t* len, int B, int64_t n_cap, float voxel, int key_bits_hint,
                            float* out_xyz, int64_t* out_len, uint32_t* status,
                            void* ws, size_t ws_bytes, void* stream);
/* HOST helper (no GPU): order[j] = insertion rank of the j-th element that libstdc++'s
 * std::unordered_map<size_t,...> visits after inserting the n distinct keys in the given order — the serial mirror of
 * the device kernel that fixes lcr_grid_subsample's output order (grid_subsampling_cpu.cpp:26,45-47). */
int lcr_hashmap_order_host(const uint64_t* keys_host, int64_t n, int64_t* order_host);
/* HOST helper (no GPU): out_host[i] = codes_host[i] mod the phase-th bucket count of libstdc++'s prime schedule (13, 29, ..., phase
 * 0..27), through the exact multiply-high reduction the device replay uses for keys of 2^52 and more. */
int lcr_hashmap_bucket_host(const uint64_t* codes_host, int64_t n, int phase, int64_t* out_host);

/* ------------------------------------------------------------------------------------------------
 * a-1o  Open3D voxel down-sampling — replaces PointCloud::VoxelDownSample (legacy Open3D, with AccumulatedPoint and
 *       utility::hash_eigen), the offline step of data/Kitti/downsample_pcd.py:29, data/Kitti_360/downsample_pcd.py and
 *       data/mulran/downsample_pcd_mulran.py, and of the helper voxel_downsample (utils/utils/open3d.py:61-69).
 * Per cloud, on rows of R = row_floats (3 .. 64) floats with x, y, z first and a voxel size v given as a DOUBLE:
 *   m      = component-wise min of the cloud's xyz (fp32 -> fp64 is exact);
 *   o      = m - v * 0.5 in fp64;
 *   i_d    = (int) floor((p_d - o_d) / v): fp64 subtract, then a true fp64 division (no reciprocal, no contraction);
 *   code   = hash_eigen(ix, iy, iz): s = 0, then for e in (ix, iy, iz): s ^= (uint64)(int64)e + 0x9e3779b9 + (s << 6) + (s >> 2) mod 2^64;
 *   voxel  = count n and fp64 sums of x, y, z and of every other output column, added in input-row order;
 *   output = sum / (double) n (a true division), rounded to fp32 (RNE) in out_f32; out_f64 (nullable) gets the unrounded averages;
 *   order  = libstdc++ std::unordered_map iteration order with the voxels inserted in first-occurrence order, bucket = code mod
 *            bucket_count.
 * Columns 3 .. out_cols-1 are averaged like an Open3D colour channel: [N,4] -> [M,4] is the KITTI `downsampled_xyzi` record
 * (intensity carried as colour channel 0), [N,4] -> [M,3] MulRan's xyz-only file.
 * hash_eigen CODES COLLIDE: it is boost's hash_combine on small integers, e.g. (1, 65, z) and (2, 2, z) share a code for every z; on
 * synthetic raw scans 4-25 % of the voxels share their code with another voxel (groups of up to 5).  Voxels are identified by their index triple (the sort key packs
 * ix + NX iy + NX NY iz with the cloud id), never by the code; distinct voxels with equal codes share a bucket, and libstdc++ puts a
 * new node at the front of its bucket whatever the codes are, which the replay reproduces.
 *   rows     f32[n_cap, row_floats]   stacked clouds (first sum(len) rows are used); len i64[B], B <= 64
 *   out_f32  f32[n_cap, out_cols]     3 <= out_cols <= row_floats; first sum(out_len) rows are written
 *   out_f64  f64[n_cap, out_cols]     or NULL
 *   status   u32[1]  LCR_STATUS_KEY_OVERFLOW when a cloud's packed index key with the cloud id needs more than key_bits_hint bits
 *            (retry with 0) or more than 64, or an axis spans INT_MAX voxels or more (Open3D refuses such clouds too): the rows are
 *            then not meaningful.  LCR_STATUS_LEN_MISMATCH: sum(len) > n_cap.
 * ------------------------------------------------------------------------------------------------ */
int lcr_voxel_down_sample_ws_bytes(int64_t n_cap, int B, size_t* bytes);
int lcr_voxel_down_sample(const float* rows, int row_floats, int out_cols, const int64_t* len, int B, int64_t n_cap, double voxel,
                          int key_bits_hint, float* out_f32, double* out_f64, int64_t* out_len, uint32_t* status,
                          void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a-1t  training augmentation and point-limit sampling — what the training datasets apply per cloud in NumPy
 *       (datasets/registration/kitti/dataset.py:73-115 `_augment_point_cloud` / `_load_point_cloud`,
 *       datasets/loop_detection/kitti/dataset_overlap_online.py:123-153), for B = 1 .. 128 stacked clouds in one call.
 * Random words are Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key increments 0x9E3779B9 / 0xBB67AE85) with
 *   key     = (low, high) half of `seed`;
 *   counter = (ORIGINAL index of the point inside its cloud, 0, sample_id[b], stream), stream 0 = noise, stream 1 = selection;
 *   uniform = (word >> 8) * 2^-24 in fp32; words 0 .. 2 of stream 0 are the uniforms of x, y, z.
 * Per kept point, fp32, every operation rounded once (no contraction), in this order:
 *   n   = p + (u - 0.5) * noise[b]                 (the product first)
 *   r_i = (R_i0 n_x + R_i1 n_y) + R_i2 n_z         (R = rotation[b], row-major)
 *   out = r * scale[b] + shift[b]
 * Point limit (`limit` <= 0: none, and no sort is launched): a cloud of L <= limit points passes through in its order; a longer
 * one keeps the `limit` points with the smallest (word 0 of stream 1, original index) pairs, written in ascending pair order —
 * one stable radix sort per call with the cloud number above the 32 random bits.  out_len[b] = min(L, limit).
 * Because the counter holds sample_id and the original index, a cloud gives the same bytes alone and inside any stack, and the
 * augmented value of source point i does not depend on `limit`.  Columns 3 .. row_floats-1 are not read (the reference returns [:, :3]).
 *   rows       f32[n_cap, row_floats]  3 <= row_floats <= 64, x, y, z first; len i64[B]; n_cap <= 2^31-2
 *   sample_id  u32[B]; rotation f32[B,9]; scale f32[B]; shift f32[B,3]; noise f32[B]
 *   out_xyz    f32[out_cap,3], 0 <= out_cap <= n_cap: the first sum(out_len) rows are written, none at or beyond out_cap
 *   out_len    i64[B]
 *   status     u32[1]  LCR_STATUS_LEN_MISMATCH: a negative length, sum(len) > n_cap or sum(out_len) > out_cap (lengths are clamped)
 * Every refusal of this entry — a too-small workspace included — is LCR_EARG with text, before any launch.
 * ------------------------------------------------------------------------------------------------ */
int lcr_augment_clouds_ws_bytes(int64_t n_cap, int B, int64_t limit, size_t* bytes);
int lcr_augment_clouds(const float* rows, int row_floats, const int64_t* len, int B, int64_t n_cap, const uint32_t* sample_id,
                       const float* rotation, const float* scale, const float* shift, const float* noise, uint64_t seed, int64_t limit,
                       float* out_xyz, int64_t out_cap, int64_t* out_len, uint32_t* status,
                       void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a-2  radius search — replaces utils.ext.radius_neighbors + the [:, :limit] slice of
 *      modules/ops/radius_search.py:7-27 (radius_neighbors.cpp:5-68 → radius_neighbors_cpu.cpp:3-91).
 * For every query: supports of the SAME cloud with d2 < radius*radius (fp32, d2 = ((dx*dx)+dy*dy)+dz*dz,
 * no FMA), ascending by (d2, index), global support index, padded with sum(slen).
 *   q f32[nq_cap,3], s f32[ns_cap,3], qlen/slen i64[B]
 *   limit > 0 : out_idx64 / out_idx32 are [nq_cap, limit] (either may be NULL)
 *   limit == 0: count only (out_cnt required)
 *   out_cnt   i32[nq_cap] uncapped in-radius count per query (NULL allowed when limit > 0)
 * lcr_support_grid_build + lcr_radius_query split the call so one grid serves several query sets.
 * ------------------------------------------------------------------------------------------------ */
int lcr_support_grid_ws_bytes(int64_t ns_cap, int B, size_t* bytes);
int lcr_support_grid_build(const float* s, const int64_t* slen, int B, int64_t ns_cap, float radius,
                           uint32_t* status, void* grid_ws, size_t grid_ws_bytes, void* stream);
int lcr_radius_query(const float* q, const int64_t* qlen, int B, int64_t nq_cap,
                     const void* grid_ws, int64_t ns_cap /* as passed to the build */, float radius, int limit,
                     int64_t* out_idx64, int32_t* out_idx32, int32_t* out_cnt, void* stream);
/* lcr_radius_query with a processing order for the queries (q_order i32[nq]: a permutation of the query rows, e.g. the query set's
 * own cell order from lcr_support_grid_build_ex; NULL = row order).  Results are identical; spatially coherent wavefronts re-use
 * their candidate cells from cache. */
int lcr_radius_query_ordered(const float* q, const int64_t* qlen, int B, int64_t nq_cap,
                             const void* grid_ws, int64_t ns_cap, float radius, int limit,
                             int64_t* out_idx64, int32_t* out_idx32, int32_t* out_cnt, const int32_t* q_order, void* stream);
/* Several searches (<= 12) of one collate in ONE launch: the ten searches of precompute_data_stack_mode (data.py:28-66) run against
 * four grids; alone, the coarse-stage ones are a handful of workgroups on the launch floor.  int32 rows only (limit >= 1), same
 * rows as lcr_radius_query_ordered search by search.  All searches share the cloud count B. */
typedef struct LcrRadiusQuery {
    const float*   q;          /* [nq_cap,3] */
    const int64_t* qlen;       /* [B] device */
    int64_t        nq_cap;
    const void*    grid_ws;    /* a built support grid */
    int64_t        ns_cap;     /* as passed to its build */
    float          radius;
    int            limit;
    int32_t*       out_idx32;  /* [nq_cap, limit] */
    const int32_t* q_order;    /* processing order or NULL */
} LcrRadiusQuery;
#define LCR_RADIUS_QUERY_MULTI_MAX 12   /* searches per lcr_radius_query_multi launch; longer lists: call it on slices */
int lcr_radius_query_multi(const LcrRadiusQuery* list, int n, int B, void* stream);
/* Same build that also writes the cell-sorted processing order (what lcr_support_grid_order returns) into order i32[ns_cap]. */
int lcr_support_grid_build_ex(const float* s, const int64_t* slen, int B, int64_t ns_cap, float radius,
                              uint32_t* status, void* grid_ws, size_t grid_ws_bytes, int32_t* order, void* stream);
/* order[i] = stacked row of the i-th support in cell-sorted order (a spatially coherent processing order for gather kernels). */
int lcr_support_grid_order(const void* grid_ws, int64_t ns_cap, int B, int32_t* order, void* stream);
int lcr_radius_search_ws_bytes(int64_t nq_cap, int64_t ns_cap, int B, size_t* bytes);
int lcr_radius_search(const float* q, const float* s, const int64_t* qlen, const int64_t* slen, int B,
                      int64_t nq_cap, int64_t ns_cap, float radius, int limit,
                      int64_t* out_idx64, int32_t* out_idx32, int32_t* out_cnt, uint32_t* status,
                      void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a-3  the whole per-batch pre-processing — replaces precompute_data_stack_mode (experiments/lcrnet/data.py:10-74: the
 *      subsampling loop :20-29 and the 10 searches :33-69) for a stack of B clouds, as ONE native call: 3 grid subsamples,
 *      4 support grids and up to 10 radius searches issued fork-join over side streams, voxel counts read back at the end.
 * lcr_precompute_layout sizes the two arenas for stage-0 capacity n0 and reports where every result lives in `out`
 * (byte offsets; int32 indices padded with sum(lengths) like the reference's lists; stage-0 points are the input itself).
 * lcr_precompute_batch: points0 f32[n0,3] and lengths0 i64[B] on the device; voxel_size is stage 0's (stage i uses
 * voxel_size * 2^i, radius * 2^i, data.py:28,73); lengths_host i64[num_stages*B] and status_host (LCR_STATUS_* bits) are
 * HOST outputs — the call returns after synchronising `stream`.  LCR_STATUS_KEY_OVERFLOW: retry with key_bits_hint = 0.
 * ------------------------------------------------------------------------------------------------ */
#define LCR_MAX_STAGES 8
typedef struct LcrPrecomputeLayout {
  int     num_stages, B, upsampling;
  int64_t n_raw;                               /* > 0: the input is a stack of RAW scans, voxelised first (stage 0 lives in `out`) */
  int     limits[LCR_MAX_STAGES];
  int64_t cap[LCR_MAX_STAGES];                 /* row capacity of every stage-i array */
  size_t  off_points[LCR_MAX_STAGES];          /* f32[cap,3]            (i >= 1; i == 0 too in raw mode: f32[n_raw,3]) */
  size_t  off_lengths[LCR_MAX_STAGES];         /* i64[B]                (i >= 1; i == 0 too in raw mode) */
  size_t  off_order[LCR_MAX_STAGES];           /* i32[cap]  cell-sorted processing order */
  size_t  off_neighbors[LCR_MAX_STAGES];       /* i32[cap, limits[i]] */
  size_t  off_subsampling[LCR_MAX_STAGES];     /* i32[cap, limits[i]]   rows = stage i+1 points (i < num_stages-1) */
  size_t  off_upsampling[LCR_MAX_STAGES];      /* i32[cap, limits[i+1]] rows = stage i points   (i < num_stages-1, if enabled); upsampling == 2: i32[cap, 1] */
  size_t  out_bytes, ws_bytes;
} LcrPrecomputeLayout;
/* n_raw > 0: raw-scan mode — the input of lcr_precompute_batch is then f32[n_raw,3] raw points + i64[B] raw lengths, voxelised
 * with `raw_voxel` (replaces the offline Open3D step) into stage 0 inside the same call; n0 is the CAPACITY
 * assumed for the voxel count (LCR_STATUS_LEN_MISMATCH in status_host if it was too small: retry with n0 = n_raw).
 * upsampling: 0 = no upsampling lists (descriptor-only deployment), 1 = the reference collate's full rows [n_i, limits[i+1]], 2 = NEAREST-ONLY
 * lists [n_i, 1]: column 0 of the full rows, which is all KPDecoder reads (nearest_upsample, backbone4.py:355-367; modules/kpconv/functional.py:21). */
int lcr_precompute_layout(int64_t n0, int B, int num_stages, const int* limits, int upsampling, int64_t n_raw,
                          LcrPrecomputeLayout* layout);
int lcr_precompute_batch(const float* points0, const int64_t* lengths0, const LcrPrecomputeLayout* layout, float voxel_size,
                         float radius, float raw_voxel, int key_bits_hint, void* out, size_t out_bytes, void* ws, size_t ws_bytes,
                         int64_t* lengths_host, uint32_t* status_host, void* stream);
/* raw-scan mode on rows of `raw_row_floats` floats (x, y, z first; 4 = KITTI velodyne [N,4] as loaded from a .bin / xyzi .npy file and
 * uploaded unsliced): points0 is then f32[n_raw, raw_row_floats].  raw_row_floats = 3 is lcr_precompute_batch. */
int lcr_precompute_batch_rows(const float* points0, int raw_row_floats, const int64_t* lengths0, const LcrPrecomputeLayout* layout,
                              float voxel_size, float radius, float raw_voxel, int key_bits_hint, void* out, size_t out_bytes, void* ws,
                              size_t ws_bytes, int64_t* lengths_host, uint32_t* status_host, void* stream);
/* Raw-scan mode with a choice of voxeliser: raw_method 0 = grid subsampling (lcr_precompute_batch_rows, raw_voxel narrowed to
 * float), 1 = Open3D VoxelDownSample (lcr_voxel_down_sample with raw_voxel as given, stage 0 = its fp32 [M,3] rows).  The workspace
 * must hold lcr_precompute_ws_bytes_ex(layout, raw_method) bytes (layout->ws_bytes is the raw_method 0 size). */
int lcr_precompute_ws_bytes_ex(const LcrPrecomputeLayout* layout, int raw_method, size_t* bytes);
int lcr_precompute_batch_rows_ex(const float* points0, int raw_row_floats, const int64_t* lengths0, const LcrPrecomputeLayout* layout,
                                 float voxel_size, float radius, double raw_voxel, int raw_method, int key_bits_hint, void* out,
                                 size_t out_bytes, void* ws, size_t ws_bytes, int64_t* lengths_host, uint32_t* status_host, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a-4 / a-5 / a-6  KPConv encoder building blocks (fp32).  Index tensors are [M,H] int32 or int64 (idx_is_64),
 * padded with Ns like the reference's neighbour lists; feature tensors are row-major [N,C].
 * ------------------------------------------------------------------------------------------------ */
/* C = A·B on the fp32 matrix cores with fused epilogue: C[m][:] = (A·B)[m][:] / rowdiv[m] + bias, and per-(segment,group)
 * sum / sum-of-squares of C ADDED to stats[LCR_GN_REPLICAS,S,groups,2] (fp64; the caller zeroes the table — one fill per
 * forward pass can cover every layer's table; consumers add the replicas — they
 * only spread same-address atomics) for the GroupNorm that follows.
 * transA: A is stored [K,M]; transB: B is stored [N,K] (nn.Linear weight).  Replaces F.linear + the (15,C,Cout)
 * contraction of KPConv.forward (modules/kpconv/kpconv.py:108-116) and torch.matmul in NetVlad.py:56,68. */
int lcr_gemm_f32(const float* A, const float* B, float* C, int64_t M, int N, int K, int transA, int transB,
                 const float* bias, const float* rowdiv, const int64_t* seg_len, int S, int groups, double* stats,
                 void* stream);
/* The K-deep contractions on the bf16 matrix cores with fp32-faithful operands: an fp32 number is exactly the sum of three bf16 numbers.
 * lcr_split_bf16x3 writes those terms of an array as planes u16[3][n]; lcr_split_bf16x3_tiles writes them for a constant operand (weights
 * [N,K], K % 32 == 0) in the order the GEMM's matrix instructions read them — ceil(N/64) * (K/32) blocks of 12288 bytes, one per (64 columns,
 * K-step of 32), each [column quarter wn 0..3][plane 0..2][lane 0..63] 16-byte chunks, lane l holding 8 bf16 of column 16 wn + (l & 15),
 * k 8 (l >> 4) .. + 7; rows beyond N are zero; opaque to callers — once;
 * lcr_gemm_f32_bsplit computes C = A[M,K] . B[N,K]^T with A split on the fly and six of the nine cross products (the dropped ones are
 * <= 2^-24 of a product), fp32 accumulation, same epilogue as lcr_gemm_f32.  Not bit-identical to lcr_gemm_f32 (other rounding points). */
int lcr_split_bf16x3(const float* w, int64_t n, uint16_t* planes, void* stream);
int lcr_split_bf16x3_tiles(const float* w, int N, int K, uint16_t* tiles, void* stream);
int lcr_gemm_f32_bsplit(const float* A, const uint16_t* Bs_tiles, float* C, int64_t M, int N, int K, const float* bias, const float* rowdiv,
                        const int64_t* seg_len, int S, int groups, double* stats, void* stream);
/* The KPConv contraction over a row-masked A (lcr_kpconv_aggregate_mask): the columns [k*block_k, (k+1)*block_k) of row m are read as
 * zeros when bit k of row_mask[m] is clear, without touching memory there.  block_k = 32 << s (32 ... 256), K <= 16 * block_k.
 * Results are bit-identical to the unmasked call on an A whose masked blocks hold zeros.
 * lcr_gemm_f32_masked: C = A[M,K] . B[N,K]^T on the K-deep fp32 form (needs K % 32 == 0 and M*K, N*K < 2^30);
 * lcr_gemm_f32_bsplit_masked: lcr_gemm_f32_bsplit's split-bf16 form (needs M*K < 2^29).  Epilogues as lcr_gemm_f32. */
int lcr_gemm_f32_masked(const float* A, const float* B, float* C, int64_t M, int N, int K, const float* bias, const float* rowdiv,
                        const int64_t* seg_len, int S, int groups, double* stats, const uint16_t* row_mask, int block_k, void* stream);
int lcr_gemm_f32_bsplit_masked(const float* A, const uint16_t* Bs_tiles, float* C, int64_t M, int N, int K, const float* bias,
                               const float* rowdiv, const int64_t* seg_len, int S, int groups, double* stats, const uint16_t* row_mask,
                               int block_k, void* stream);
/* 1 when the contraction of a KPConv aggregate [M, K = 15 C] with N outputs may run on the masked entry above (split = 1: the split-bf16
 * form, 0: the fp32 form) and give what the unmasked call gives; 0 otherwise, and always with environment LCR_KP_MASK=0. */
int lcr_kpconv_mask_ok(int64_t M, int N, int K, int split);
/* C = LeakyReLU(GroupNorm(A)) · B^T (+ bias, + statistics of C as above), A being the RAW [M,K] output of the layer whose sums are
 * a_stats[LCR_GN_REPLICAS,S,a_groups,2]: the normalisation happens while A's tiles are staged, the normalised tensor never
 * exists in memory.  Replaces norm_conv + leaky_relu + unary2.mlp of ResidualBlock.forward (modules/kpconv/modules.py:215-217).
 * Needs B stored [N,K] (nn.Linear weight), 32 < N, K <= 256, K % 4 == 0, a segment table (S >= 1) whose segments all hold >= 64
 * rows (the caller's guarantee: a 64-row block then touches at most two segments).  LCR_EARG outside that form. */
int lcr_gemm_f32_anorm(const float* A, const float* B, float* C, int64_t M, int N, int K, const float* bias,
                       const double* a_stats, const float* a_gamma, const float* a_beta, int a_groups, float a_eps,
                       float a_slope, const int64_t* seg_len, int S, int groups, double* stats, void* stream);
/* The same on the split-bf16 form: B given as the tiled planes of lcr_split_bf16x3_tiles, A normalised and THEN split while its tiles are
 * staged (the normalised operand is bit-equal to lcr_gemm_f32_anorm's).  Needs N >= 64, 32 <= K <= 256, K % 32 == 0, the segment table as
 * above.  LCR_EARG (with text, no launch) outside that form. */
int lcr_gemm_f32_bsplit_anorm(const float* A, const uint16_t* Bs_tiles, float* C, int64_t M, int N, int K, const float* bias,
                              const double* a_stats, const float* a_gamma, const float* a_beta, int a_groups, float a_eps,
                              float a_slope, const int64_t* seg_len, int S, int groups, double* stats, void* stream);
/* 1 when a Linear with N outputs and K inputs runs on the split-bf16 form wherever the caller has the weight's planes (the encoder driver's
 * and the module tree's one dispatch rule, a function of (N, K) alone): N >= 64, K % 32 == 0 and K >= 288, or one of the K <= 256 classes
 * that measured faster there (environment LCR_GEMM_SPLIT_LIGHT=0: none of those).  0 otherwise. */
int lcr_gemm_split_ok(int N, int K);
/* K-deep problems (A [M,K] x B [K,N], K >= 480) whose 64x64 tiles do not divide evenly over the CUs can run as stream-K (opt-in,
 * environment LCR_GEMM_STREAMK; scratch library-owned, one per stream; hook: lcr_gemm_debug_streamk in lcr_hip_debug.h). */
/* Batched C_z[M,N] = A_z^T · B_z with A_z stored [K_z, M] (per-entry K and element offsets, HOST arrays, count <= 64). */
int lcr_gemm_f32_batched_ta(const float* A, const float* B, float* C, int64_t M, int N, int count, const int* k_host,
                            const int64_t* a_off_host, const int64_t* b_off_host, const int64_t* c_off_host, void* stream);
/* Gather + kernel-point influences + weighted aggregation of KPConv.forward (kpconv.py:91-105): A[m][k*C+c] =
 * sum_h max(0, 1-|s[idx[m,h]]-q[m]-kp[k]|/sigma) * s_feats[idx[m,h]][c];  nn[m] = max(1, #neighbours with s_pos != 0)
 * (kpconv.py:113-116).  kernel_points_host: 15x3 floats in HOST memory.  C in {32,64,128,256}, H <= 128. */
int lcr_kpconv_aggregate(const float* s_feats, const uint8_t* s_pos, const float* q_pts, const float* s_pts,
                         const void* idx, int idx_is_64, int64_t M, int64_t Ns, int H, int C,
                         const float* kernel_points_host, float sigma, float* A, float* nn,
                         const int32_t* order /* optional i32[M]: processing order, e.g. lcr_support_grid_order */, void* stream);
/* Same with flags.  LCR_KP_VALID_FIRST: the caller guarantees that every row of idx holds its valid entries first and the padding (any value
 * outside [0, Ns)) behind them — what a radius search emits (radius_neighbors_cpu.cpp:70-88 pads behind the sorted hits); the kernel then
 * stops reading a row at the first 64-column chunk that contains padding.  Results are identical for such rows. */
#define LCR_KP_VALID_FIRST 1
int lcr_kpconv_aggregate_ex(const float* s_feats, const uint8_t* s_pos, const float* q_pts, const float* s_pts,
                            const void* idx, int idx_is_64, int64_t M, int64_t Ns, int H, int C,
                            const float* kernel_points_host, float sigma, float* A, float* nn,
                            const int32_t* order, int flags, void* stream);
/* Same, and mask[M] (uint16): bit k of mask[m] is set when the kernel-point block A[m, k*C : (k+1)*C] holds a value other than +0 / -0
 * (NaN and Inf included).  Only those blocks are STORED; the others are left as they were, to be read through
 * lcr_gemm_f32_masked / lcr_gemm_f32_bsplit_masked, which zero-fill them.  mask = NULL: lcr_kpconv_aggregate_ex. */
int lcr_kpconv_aggregate_mask(const float* s_feats, const uint8_t* s_pos, const float* q_pts, const float* s_pts,
                              const void* idx, int idx_is_64, int64_t M, int64_t Ns, int H, int C,
                              const float* kernel_points_host, float sigma, float* A, float* nn, uint16_t* mask,
                              const int32_t* order, int flags, void* stream);
/* Whole KPConv (kpconv.py:79-122) for C_in = C_out = 32 — the two widest query sets of the encoder — in one launch: the
 * aggregate above lives only as 16-query tiles in LDS and is contracted there with W [15*32, 32] (split-K over the wavefronts,
 * weights in registers); out[M,32] = contraction / neighbour count + bias, plus the GroupNorm sums of `out` ADDED to
 * stats[LCR_GN_REPLICAS,S,groups,2] (optional; S <= 64).  Same results as lcr_kpconv_aggregate + lcr_gemm_f32 up to fp32
 * summation order. */
int lcr_kpconv_fused(const float* s_feats, const uint8_t* s_pos, const float* q_pts, const float* s_pts, const void* idx,
                     int idx_is_64, int64_t M, int64_t Ns, int H, int C, const float* kernel_points_host, float sigma,
                     const float* W, const float* bias, float* out, const int64_t* seg_len, int S, int groups, double* stats,
                     const int32_t* order, void* stream);
/* Whole KPConv for C_in = 1 (encoder1_1, backbone4.py:15): out[M,Cout] incl. count normalisation and bias. W: [15,Cout]. */
int lcr_kpconv_cin1(const float* s_feats, const float* q_pts, const float* s_pts, const void* idx, int idx_is_64,
                    int64_t M, int64_t Ns, int H, const float* kernel_points_host, float sigma, const float* W,
                    const float* bias, int Cout, float* out, const int32_t* order, void* stream);
/* maxpool over neighbours, zero shadow row (modules/kpconv/functional.py:54-67). */
int lcr_maxpool(const float* x, const void* idx, int idx_is_64, int64_t M, int64_t Ns, int H, int C, float* out,
                const int32_t* order, void* stream);
/* pos[n] = (sum_c x[n][c] > 0) — the flag behind KPConv's neighbour count. */
int lcr_row_positive(const float* x, int64_t N, int C, uint8_t* pos, void* stream);
/* Segmented GroupNorm statistics (sum, sumsq per segment and group, fp64, [LCR_GN_REPLICAS,S,groups,2]) of x[N,C],
 * ADDED to the caller-zeroed table. */
int lcr_groupnorm_stats(const float* x, int64_t N, int C, int groups, const int64_t* seg_len, int S, double* stats, void* stream);
/* y = act( GN(x; stats,gamma,beta) [+ res | + GN(res; res_stats,res_gamma,res_beta)] ), act = LeakyReLU(slope) if act != 0
 * (modules/kpconv/modules.py:33-50, 78-84, 207-225).  Optional pos[n] = (sum_c y[n][c] > 0). */
int lcr_groupnorm_apply(const float* x, const double* stats, const float* gamma, const float* beta, const float* res,
                        const double* res_stats, const float* res_gamma, const float* res_beta, float* y, int64_t N, int C,
                        int groups, const int64_t* seg_len, int S, float eps, float slope, int act, uint8_t* pos, void* stream);

/* Reverse passes of the encoder block above (csrc/kpconv_grad.hip, csrc/groupnorm_grad.hip).  None of them changes what the forward entries
 * compute.  They are gathers over an INVERTED neighbour list and two-stage sums with a fixed order: no floating-point atomics, results
 * repeat to the bit, and a cloud's rows get the same bytes alone and inside a stack.  Index lists: int32 or int64 (idx_is_64), padding =
 * any index outside [0, Ns); H <= 128 and M * H < 2^30.  A call outside the domain returns LCR_EARG with text and launches nothing.
 *
 * lcr_neighbor_transpose: idx [M,H] -> row_start i32[Ns + 1], edges u32[row_start[Ns]] (capacity M * H).  The edges of support row n,
 * edges[row_start[n] : row_start[n + 1]], are the flat positions m * H + h with idx[m,h] == n in ascending order (the stable radix sort of
 * csrc/radix_sort.h on (support index, flat position)); padding entries appear nowhere.  ws: lcr_neighbor_transpose_ws_bytes(M, H), host-only. */
int lcr_neighbor_transpose_ws_bytes(int64_t M, int H, size_t* bytes);
int lcr_neighbor_transpose(const void* idx, int idx_is_64, int64_t M, int64_t Ns, int H, int32_t* row_start, uint32_t* edges,
                           void* ws, size_t ws_bytes, void* stream);
/* Reverse of lcr_kpconv_aggregate to s_feats: d_s_feats[n][c] = sum over the edges (m,h) of n, sum_k w(m,h,k) dA[m][k*C + c], with the
 * forward's influence w = max(0, 1 - |s_n - q_m - kp_k| / sigma) evaluated operation for operation as the forward does.  dA [M,15*C];
 * C in {32, 64, 128, 256}.  Only the kernel-point blocks of dA with a non-zero influence are read.  A support nobody lists gets zeros. */
int lcr_kpconv_aggregate_grad(const float* dA, const float* q_pts, const float* s_pts, const int32_t* row_start, const uint32_t* edges,
                              int64_t M, int64_t Ns, int H, int C, const float* kernel_points_host, float sigma, float* d_s_feats,
                              void* stream);
/* Reverse of lcr_kpconv_cin1: dW [15,Cout] and dbias [Cout] (may be NULL) from d_out [M,Cout], per-workgroup partials added in ascending
 * order.  nn: the forward's neighbour count per query, or NULL (recounted from s_feats > 0; at least 1 either way).  d_s_feats [Ns] is
 * optional (NULL: skipped, row_start / edges may then be NULL too).  ws: lcr_kpconv_cin1_grad_ws_bytes(M, Cout, d_s_feats != NULL). */
int lcr_kpconv_cin1_grad_ws_bytes(int64_t M, int Cout, int want_feats, size_t* bytes);
int lcr_kpconv_cin1_grad(const float* d_out, const float* s_feats, const float* q_pts, const float* s_pts, const void* idx, int idx_is_64,
                         const float* nn, const int32_t* row_start, const uint32_t* edges, int64_t M, int64_t Ns, int H,
                         const float* kernel_points_host, float sigma, const float* W, int Cout, float* dW, float* dbias,
                         float* d_s_feats, void* ws, size_t ws_bytes, void* stream);
/* Reverse of lcr_maxpool: d_x[n][c] = sum of d_out[m][c] over the edges (m,h) of n for which h is the FIRST real entry of row m with
 * x[idx[m,h]][c] == pooled[m][c] (pooled = the forward's output); a maximum owned by the zero shadow row sends its gradient nowhere.
 * winners u8[M,C] is written by a first pass (the winning column, 255 = none) and may be discarded afterwards. */
int lcr_maxpool_grad(const float* d_out, const float* x, const float* pooled, const void* idx, int idx_is_64, const int32_t* row_start,
                     const uint32_t* edges, int64_t M, int64_t Ns, int H, int C, uint8_t* winners, float* d_x, void* stream);
/* Reverse of lcr_kpconv_aggregate to the POINTS (csrc/kpconv_grad.hip).  dA [M,15*C] as above, s_feats [Ns,C], idx the forward's list.  With
 * e = s_n - q_m - kp_k, r = |e|, t(m,h,k) = sum_c dA[m][k*C + c] s_feats[idx[m,h]][c] and v(m,h) = sum over the k with 0 < r < sigma of
 * t e / (sigma r):  d_q[m] = sum_h v(m,h) in column order, d_s[n] = -(sum of v over the edges of n, in inverted-list order).  Either output
 * may be NULL; d_s needs row_start / edges (lcr_neighbor_transpose), d_q alone does not.  Whether an edge is live (w > 0) is decided by the
 * forward's own arithmetic; a term with r == 0 is DEFINED as zero (the self edge of a cloud convolved with itself does not move
 * with the point), a term with w == 0 and a padding entry contribute exactly 0.  q_pts and s_pts may be the same tensor: the caller adds
 * d_q and d_s.  C in {32, 64, 128, 256}.  M == 0 or Ns == 0: a no-op apart from zero-filling the output that has rows.
 * ws: lcr_kpconv_points_grad_ws_bytes(M, H) (v [M,H,3]; host-only query). */
int lcr_kpconv_points_grad_ws_bytes(int64_t M, int H, size_t* bytes);
int lcr_kpconv_points_grad(const float* dA, const float* s_feats, const float* q_pts, const float* s_pts, const void* idx, int idx_is_64,
                           const int32_t* row_start, const uint32_t* edges, int64_t M, int64_t Ns, int H, int C,
                           const float* kernel_points_host, float sigma, float* d_q, float* d_s, void* ws, size_t ws_bytes, void* stream);
/* Reverse of lcr_groupnorm_apply, including the path through the statistics.  x: the raw input, stats: the forward's own table, y: the
 * forward's output (read for the LeakyReLU mask only; may be NULL when act == 0), dy [N,C].  With dz = dy * (y > 0 ? 1 : slope) (act) or dy,
 * x^ = (x - mean) * rstd and g = dz * gamma: dbeta[c] = sum_n dz, dgamma[c] = sum_n dz x^, dx = rstd * (g - mean_sg(g) - x^ mean_sg(g x^)), the
 * means over the elements of one (segment, group); mean and rstd are derived from the table exactly as the forward derives them.  dz
 * (optional) is the gradient of a plain residual; for a normalised residual call again on dz with act = 0 and the residual's table.
 * dgamma / dbeta may be NULL.  C % 4 == 0, C % groups == 0, C <= 2048, S <= 256.  ws: lcr_groupnorm_apply_grad_ws_bytes(N, C, groups, S). */
int lcr_groupnorm_apply_grad_ws_bytes(int64_t N, int C, int groups, int S, size_t* bytes);
int lcr_groupnorm_apply_grad(const float* x, const double* stats, const float* gamma, const float* y, const float* dy, int64_t N, int C,
                             int groups, const int64_t* seg_len, int S, float eps, float slope, int act, float* dx, float* dgamma,
                             float* dbeta, float* dz, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a-6  the whole KPEncoder.forward (experiments/lcrnet/backbone4.py:60-89: encoder1_1 ... encoder4_3) as ONE native call: the
 *      host-side sequencer over the building blocks above (same launches, arguments and order as the module tree of
 *      modules/kpconv/modules.py:104-225, so the outputs are bit-identical to calling the blocks one by one).
 * Weights are device pointers into the model's own parameter tensors (nothing is copied or repacked); kernel points are HOST
 * float[15*3] arrays.  A NULL `w` in a unary block means nn.Identity (modules.py:171,176).
 *   points[4] f32[n_i,3]; neighbors[4] i32[n_i, limits[i]]; subsampling[3] i32[n_{i+1}, limits[i]]; order[4] i32[n_i] or NULL;
 *   seg_len[4] i64[S] GroupNorm segments per stage (device); n_host[4], limits[4] on the host; feats0 f32[n_0] (C_in = 1);
 *   seg_min_rows_host[4] (or NULL): rows of the shortest segment per stage as the host knows them, 0 = unknown — with >= 64
 *   the in-block norm_conv pass is folded into unary2's GEMM (lcr_gemm_f32_anorm), otherwise it is a launch of its own;
 *   out_feats[4]: f32[n_0,2d], [n_1,4d], [n_2,8d], [n_3,16d] (d = init_dim) — the four stage outputs (feats_list).
 * ------------------------------------------------------------------------------------------------ */
#define LCR_ENC_BLOCKS 10
typedef struct LcrUnaryW {
  const float *w, *b;          /* nn.Linear weight [cout,cin], bias [cout] */
  const float *gn_w, *gn_b;    /* GroupNorm affine [cout] */
  const uint16_t* w_split;     /* optional: lcr_split_bf16x3_tiles of w; used where lcr_gemm_split_ok(cout, cin) */
} LcrUnaryW;
typedef struct LcrBlockW {     /* ResidualBlock (modules.py:148-225) */
  int   cin, cout, strided;
  float sigma;
  const float* kernel_points_host;
  const float *kp_w, *kp_b;    /* KPConv weights [15, cout/4, cout/4], bias [cout/4] */
  const float* kp_wt;          /* optional: the same weights as [cout/4, 15 * cout/4] (k-contiguous rows: the K-deep GEMM form); NULL = not provided */
  const uint16_t* kp_wt_split; /* optional: lcr_split_bf16x3_tiles of kp_wt: the contraction then runs on the bf16 matrix cores (lcr_gemm_f32_bsplit; cout/4 >= 64) */
  const float *normconv_w, *normconv_b;
  LcrUnaryW unary1, unary2, shortcut;
} LcrBlockW;
typedef struct LcrEncoderW {
  int   groups, c1_cout;
  float c1_sigma;
  const float* c1_kernel_points_host;
  const float *c1_w, *c1_b;    /* encoder1_1 KPConv [15,1,c1_cout], bias */
  const float *c1_gn_w, *c1_gn_b;
  LcrBlockW blocks[LCR_ENC_BLOCKS];   /* encoder1_2, 2_1, 2_2, 2_3, 3_1, 3_2, 3_3, 4_1, 4_2, 4_3 */
} LcrEncoderW;
/* neighbors / subsampling: any [n, limit] index rows padded with the number of support rows (padding may sit anywhere in a row). */
int lcr_encoder_ws_bytes(const LcrEncoderW* W, const int64_t* n_host, int S, size_t* bytes);
int lcr_encoder_forward(const LcrEncoderW* W, const float* feats0, const float* const* points, const int32_t* const* neighbors,
                        const int32_t* const* subsampling, const int32_t* const* order, const int64_t* const* seg_len, int S,
                        const int64_t* n_host, const int64_t* seg_min_rows_host, const int* limits, float* const* out_feats, void* ws,
                        size_t ws_bytes, void* stream);
/* Same with flags.  LCR_ENC_LISTS_VALID_FIRST: the caller guarantees that every row of neighbors / subsampling holds its valid entries
 * first and the padding behind them — what a radius search emits (the reference's radius_neighbors and lcr_radius_search alike); the
 * KPConv aggregation then stops reading a row at its first chunk with a hole (LCR_KP_VALID_FIRST of lcr_kpconv_aggregate_ex).  With
 * rows that violate the promise the neighbours behind the first hole are silently ignored, hence opt-in (lcr_encoder_forward = flags 0).
 * The Python host sets it for data dictionaries built by its own collate (`lists_valid_first`).  Environment LCR_KP_VALID_FIRST=0
 * ignores the flag (A/B). */
#define LCR_ENC_LISTS_VALID_FIRST 1u
int lcr_encoder_forward_ex(const LcrEncoderW* W, const float* feats0, const float* const* points, const int32_t* const* neighbors,
                           const int32_t* const* subsampling, const int32_t* const* order, const int64_t* const* seg_len, int S,
                           const int64_t* n_host, const int64_t* seg_min_rows_host, const int* limits, float* const* out_feats,
                           unsigned flags, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a-7  global descriptor head: F.normalize -> NetVLADLoupe2 -> GatingContext -> F.normalize
 *      (model_family/LCRNet_GlobalDescrition.py:34-38, modules/netvlad/NetVlad.py:49-87, 165-201), S scans per call.
 * ------------------------------------------------------------------------------------------------ */
typedef struct LcrNetvladWeights {   /* device pointers; reference parameter names `netvlad.*` */
  const float* cluster_weights;      /* (1024, 64) */
  const float* cluster_weights2;     /* (1, 1024, 64) */
  const float* hidden1_weights;      /* (65536, 256) */
  const float *bn1_w, *bn1_b, *bn1_mean, *bn1_var;
  const float *bn2_w, *bn2_b, *bn2_mean, *bn2_var;
  const float* gating_weights;       /* (256, 256) */
  const float *gbn_w, *gbn_b, *gbn_mean, *gbn_var;
} LcrNetvladWeights;
int lcr_netvlad_ws_bytes(int64_t n_rows, int S, size_t* bytes);
int lcr_netvlad_forward(const float* feats /*[sum(seg_len),1024]*/, const int64_t* seg_len_host, int S,
                        const LcrNetvladWeights* weights_host, float* out /*[S,256]*/, void* ws, size_t ws_bytes, void* stream);
/* The head in TRAINING mode (GlobalDescritionHEAD's training branch, LCRNet_GlobalDescrition.py:40-57): every cloud stands for its cyclic
 * padding to Lmax = max(seg_len) rows — local row i of a cloud of L rows counts c = (Lmax-1-i)/L + 1 times in bn1's batch statistics (taken
 * over S*Lmax rows) and carries the assignment softmax + (c-1)/64 (padding rows are uniform) — and bn2 / context_gating.bn1 use the
 * statistics of the S descriptors.  The running_mean / running_var members of `weights_host` are not read.
 * batch_stats[1152] receives mean and BIASED variance: bn1 mean[64], var[64], bn2 mean[256], var[256], context_gating.bn1 mean[256], var[256].
 * `saved` (lcr_netvlad_train_saved_bytes) keeps what lcr_netvlad_backward reads: x.Wc and the softmax [N,64], each row's multiplicity and cloud,
 * v [S,65536] with its raw norms, the column sums of the assignment and the [S,256] tensors of the tail; the unit rows are formed again there.
 * Domain: 1 < S <= 128, every seg_len >= 1; LCR_EARG with text and no launch outside it.  Every sum has a fixed order (no atomics): the same
 * call gives the same bytes. */
typedef struct LcrNetvladGrads {     /* device pointers, shapes of the parameters; NULL = that gradient is not formed */
  float* cluster_weights;
  float* cluster_weights2;
  float* hidden1_weights;
  float *bn1_w, *bn1_b;
  float *bn2_w, *bn2_b;
  float* gating_weights;
  float *gbn_w, *gbn_b;
} LcrNetvladGrads;
int lcr_netvlad_train_ws_bytes(int64_t n_rows, int S, size_t* bytes);
int lcr_netvlad_train_saved_bytes(int64_t n_rows, int S, size_t* bytes);
int lcr_netvlad_train_forward(const float* feats /*[sum(seg_len),1024]*/, const int64_t* seg_len_host, int S,
                              const LcrNetvladWeights* weights_host, float* out /*[S,256]*/, float* batch_stats /*[1152]*/, void* saved,
                              size_t saved_bytes, void* ws, size_t ws_bytes, void* stream);
/* d_out [S,256] -> d_feats [N,1024] (NULL: skipped) and the gradients named in `grads_host`; feats, seg_len_host, weights and `saved` as in the
 * forward call.  The hidden projection's reverse is one sweep over the rows of hidden1_weights that forms dv = dh.H^T and dH = v^T.dh together. */
int lcr_netvlad_backward_ws_bytes(int64_t n_rows, int S, size_t* bytes);
int lcr_netvlad_backward(const float* d_out, const float* feats, const int64_t* seg_len_host, int S, const LcrNetvladWeights* weights_host,
                         const void* saved, size_t saved_bytes, float* d_feats, const LcrNetvladGrads* grads_host, void* ws, size_t ws_bytes,
                         void* stream);

/* ------------------------------------------------------------------------------------------------
 * a-8  3D-RoFormer attention block (fp32) — RPEMultiHeadAttention / MultiHeadAttention of
 *      modules/thdroformer/rpetransformer.py:41-108 and vanilla_transformer.py:30-118.
 * ------------------------------------------------------------------------------------------------ */
/* x[N, heads*32] <- x*cos(theta) + rot(x)*sin(theta) in place, theta[N, heads*16] (one angle per adjacent channel pair). */
int lcr_rotary_embed(float* x, const float* theta, int64_t N, int heads, void* stream);
/* out[Nq, heads*32] = softmax(q k^T / sqrt(32)) v per head, fused (no score matrix in memory); head_dim must be 32. */
int lcr_attention_f32(const float* q, const float* k, const float* v, int64_t Nq, int64_t Nk, int heads, int head_dim,
                      float* out, void* stream);
/* P (<= 64) independent attention problems in one launch over stacked q / k / v: problem p attends its q_len[p] query rows to its
 * k_len[p] key rows (HOST arrays; rows are stacked in problem order).  The batch form of RPEMultiHeadAttention /
 * MultiHeadAttention for P registration pairs per call (reference loop: model_family/LCRNet.py:274-321, one pair per forward). */
int lcr_attention_seg_f32(const float* q, const float* k, const float* v, const int64_t* q_len_host, const int64_t* k_len_host, int P,
                          int heads, int head_dim, float* out, void* stream);
/* Top-k sparsified attention — dynamic_attention with k != None (rpetransformer.py:19-39; cfg.GAT.k, None in the shipped configuration):
 * per query and head the kk_host[p] largest scores of problem p are soft-maxed, all others contribute nothing (kk = int(n_queries * k) is
 * the caller's arithmetic; ties at the threshold are taken in index order — torch.topk leaves that order unspecified).  Keys per problem
 * <= 4096. */
int lcr_attention_topk_f32(const float* q, const float* k, const float* v, const int64_t* q_len_host, const int64_t* k_len_host,
                           const int* kk_host, int P, int heads, int head_dim, float* out, void* stream);
/* y = LayerNorm(a + b) (b may be NULL), rows of D <= 1024 features. */
int lcr_add_layernorm(const float* a, const float* b, const float* gamma, const float* beta, int64_t N, int D, float eps,
                      float* y, void* stream);
int lcr_relu_inplace(float* x, int64_t n, void* stream);

/* Reverse passes of the block above (csrc/attention_grad.hip).  None of them changes what the forward entries compute or keep.
 *
 * lcr_attention_seg_grad_f32: q, k, v as the forward consumed them (post-rotary), out = the forward's result, d_out = dL/d(out) ->
 * dq [sum q_len, heads*32], dk, dv [sum k_len, heads*32].  Same domain as lcr_attention_seg_f32 (P = 1 covers lcr_attention_f32).  The
 * softmax row statistic is recomputed by the call (L = m + log2 l per query and head, with D = sum_d d_out*out, in ws:
 * lcr_attention_grad_ws_bytes(sum q_len, heads), host-only); then one kernel over key tiles (dk, dv) and one over query tiles (dq), partial
 * sums merged in a fixed order: no floating-point atomics, results repeat to the bit and a problem's bytes do not depend on its batch.  A
 * query whose d_out row is zero gets a zero dq row; with one key dq = dk = 0 and dv = d_out exactly.  A short workspace or a null pointer is
 * refused before any launch. */
int lcr_attention_grad_ws_bytes(int64_t n_queries, int heads, size_t* bytes);
int lcr_attention_seg_grad_f32(const float* q, const float* k, const float* v, const float* out, const float* d_out,
                               const int64_t* q_len_host, const int64_t* k_len_host, int P, int heads, int head_dim, float* dq, float* dk,
                               float* dv, void* ws, size_t ws_bytes, void* stream);
/* From the POST-rotary y [N, heads*32] and dy: dx = R(-theta) dy and dtheta [N, heads*16] = dy0*(-y1) + dy1*y0 per channel pair
 * (d y / d theta = rot(y): the pre-rotary tensor is not needed). */
int lcr_rotary_embed_grad(const float* y, const float* dy, const float* theta, int64_t N, int heads, float* dx, float* dtheta, void* stream);
/* y = LayerNorm(a + b) reversed: dx f32[N,D] = dL/d(a + b) (both addends receive it), dgamma, dbeta f32[D].  Mean and rstd are recomputed
 * per row; dgamma / dbeta are column sums in two stages with a fixed order (partials in ws: lcr_add_layernorm_grad_ws_bytes(N, D), host-only).
 * b may be NULL; D <= 1024; N == 0 writes zero dgamma / dbeta. */
int lcr_add_layernorm_grad_ws_bytes(int64_t N, int D, size_t* bytes);
int lcr_add_layernorm_grad(const float* a, const float* b, const float* gamma, const float* dy, int64_t N, int D, float eps, float* dx,
                           float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);

/* The whole ThDRoFormer.forward (thdroformer_linear.py:60-97: position embedding, in_proj, [self, cross] x num_layers, out_proj) as ONE native
 * call: the host-side sequencer over the entries above (same launches, arguments and order as lcr-net_amd/modules/thdroformer, so the
 * outputs are bit-identical to the module tree).  Dense attention only (cfg.GAT.k = None, the shipped configuration; the top-k form runs
 * through the module tree).  Weights are device pointers into the model's own parameters (nn.Linear layout [out,in]).
 *   points f32[n,3], feats f32[n,d_in]: the rows of all FIRST clouds of the P pairs stacked, then those of all SECOND clouds
 *   (n = sum lens0 + sum lens1; lens*_host: P entries each, 1 <= P <= 32);
 *   out f32[n,d_out] (same row order), theta_out f32[n,d_model/2] (the rotary angles, thdroformer_linear.py:94-95). */
#define LCR_ROFORMER_MAX_BLOCKS 16
typedef struct LcrLinearW {
  const float *w, *b;          /* nn.Linear weight [out,in], bias [out] */
} LcrLinearW;
typedef struct LcrRoformerLayerW {   /* _TransformerLayer: attention (proj_q/k/v, linear, norm) + output (expand, squeeze, norm) */
  LcrLinearW   q, k, v, lin;
  const float *ln1_w, *ln1_b;
  float        ln1_eps;
  LcrLinearW   expand, squeeze;
  const float *ln2_w, *ln2_b;
  float        ln2_eps;
} LcrRoformerLayerW;
typedef struct LcrRoformerW {
  int        d_in, d_model, d_out, heads, num_blocks;
  int        block_is_self[LCR_ROFORMER_MAX_BLOCKS];   /* 1 = rotary self layer over both clouds, 0 = sequential cross layer */
  LcrLinearW emb1, emb2, in_proj, out_proj;
  LcrRoformerLayerW layers[LCR_ROFORMER_MAX_BLOCKS];
} LcrRoformerW;
int lcr_roformer_ws_bytes(const LcrRoformerW* W, int64_t n_rows, size_t* bytes);
int lcr_roformer_forward(const LcrRoformerW* W, const float* points, const float* feats, const int64_t* lens0_host, const int64_t* lens1_host,
                         int P, float* out, float* theta_out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a-9  descriptor retrieval: exhaustive squared-L2 top-k with the temporal exclusion window — replaces the per-query
 *      faiss IndexIVFFlat(nlist=1) loop of experiments/loop_detection/eval_loop_detection_overlap_dataset.py:183-214.
 * Query row r is global frame q0+r; its database is frames [0, q0+r-exclude).  Rows ascending in (d2, index); short rows
 * are padded with (-1, +inf).  k <= 128.
 * ------------------------------------------------------------------------------------------------ */
int lcr_retrieval_ws_bytes(int64_t Q, int64_t C, size_t* bytes);
int lcr_retrieval_topk(const float* queries /*[Q,D]*/, int64_t Q, int64_t q0, const float* database /*[C,D]*/, int64_t C,
                       int D, int k, int exclude, int32_t* out_idx /*[Q,k]*/, float* out_d2 /*[Q,k]*/,
                       void* ws, size_t ws_bytes, void* stream);

/* Uniform batched GEMM: C_z = op(A_z)·op(B_z), constant strides in floats (multiples of 4), count <= 65535
 * (einsum('bnd,bmd->bnm') of LCRNet.py:237). */
int lcr_gemm_f32_strided_batched(const float* A, const float* B, float* C, int64_t M, int N, int K, int transA, int transB,
                                 int64_t strideA, int64_t strideB, int64_t strideC, int count, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a-10  registration tail (all device-side; replaces op chains with .cpu() hops and Python loops)
 * ------------------------------------------------------------------------------------------------ */
/* out = xyz + off * min(1, max_range/|off|)  (modules/vote/vote.py:166-175) */
int lcr_vote_shift(const float* xyz, const float* offsets, int64_t N, float max_range, float* out, void* stream);
/* Greedy NMS of modules/vote/vote.py:13-70, exact (order-dependent rule replayed in parallel rounds), one cloud per
 * workgroup.  keep u8[n_total], out_len i64[B]; ws: lcr_greedy_nms_ws_bytes(n_total). */
int lcr_greedy_nms_ws_bytes(int64_t n_total, size_t* bytes);
int lcr_greedy_nms(const float* pts, const int64_t* len, int B, int64_t n_total, float radius, uint8_t* keep,
                   int64_t* out_len, void* ws, void* stream);
/* out[m] = mean of pts[idx[m,h]] over the valid (0 <= idx < pad) neighbours (backbone4.py:161-175). */
int lcr_neighbor_mean(const float* pts, const void* idx, int idx_is_64, int64_t M, int H, int64_t pad, float* out, void* stream);
/* point_to_node_partition (modules/ops/pointcloud_partition.py:60-107): knn i64[M,K] padded with N, knn_mask u8[M,K],
 * node_mask u8[M], optional p2n i32[N]; M <= 4000. */
int lcr_point_to_node_ws_bytes(int64_t N, int M, size_t* bytes);
int lcr_point_to_node_partition(const float* points, int64_t N, const float* nodes, int M, int K, int32_t* p2n, int64_t* knn,
                                uint8_t* knn_mask, uint8_t* node_mask, uint32_t* status, void* ws, size_t ws_bytes, void* stream);

/* The same partition for C stacked clouds in one launch sequence (cloud c: points [point_off[c], point_off[c+1]), nodes
 * [node_off[c], node_off[c+1]); HOST offsets, C <= 64): per-cloud results stacked, indices local to their cloud, knn padded with the
 * cloud's own point count.  Workspace: lcr_point_to_node_ws_bytes(total points, total nodes).  The pair model's group path calls
 * this once per group of pairs instead of once per cloud (reference: ops/pointcloud_partition.py:60-107, called per cloud at
 * model_family/LCRNet.py:150-165). */
int lcr_point_to_node_partition_stack(const float* points, const int64_t* point_off, const float* nodes, const int64_t* node_off, int C, int K,
                                      int32_t* p2n_out, int64_t* knn, uint8_t* knn_mask, uint8_t* node_mask, uint32_t* status, void* ws,
                                      size_t ws_bytes, void* stream);
/* S[B,M+1,N+1] = scale*raw with dustbin row/col = alpha[0] and masked rows/cols = -inf_val (learnable_sinkhorn.py:36-45). */
int lcr_build_padded_scores(const float* raw, const uint8_t* row_mask, const uint8_t* col_mask, int64_t B, int M, int N,
                            float scale, const float* alpha, float inf_val, float* S, void* stream);
/* LearnableLogOptimalTransport.forward (learnable_sinkhorn.py:13-66) in place on S; uv_ws: B*(2*(M+N+2)+1) floats. */
int lcr_log_sinkhorn(float* S, const uint8_t* row_mask, const uint8_t* col_mask, int64_t B, int M, int N, int iters,
                     float inf_val, float* uv_ws, void* stream);
/* same with a workspace of lcr_log_sinkhorn_ws_floats(B, M, N) floats: matrices beyond LDS (the ~350 x 330 node level) then run as ONE
 * persistent launch (row slabs per workgroup, one counter hand-off per iteration) instead of two launches per iteration; the last
 * floats of the workspace hold a status word (bit 0: a hand-off timed out — the result is then invalid). */
int lcr_log_sinkhorn_ws_floats(int64_t B, int M, int N, size_t* floats);
/* which form lcr_log_sinkhorn_ex takes for (B, M, N) with a workspace of lcr_log_sinkhorn_ws_floats floats: 0 register-resident
 * (scaled / log domain), 1 LDS-resident, 2 persistent (the ONLY form that writes the status word), 3 two launches per iteration. */
int lcr_log_sinkhorn_form(int64_t B, int M, int N, int* form);
int lcr_log_sinkhorn_ex(float* S, const uint8_t* row_mask, const uint8_t* col_mask, int64_t B, int M, int N, int iters,
                        float inf_val, float* uv_ws, size_t uv_floats, void* stream);
/* Reverse pass of the transport (csrc/sinkhorn_grad.hip).  S0: the padded scores BEFORE the transport (what lcr_build_padded_scores /
 * lcr_patch_scores write), G = dL/d(output) f32[B,M+1,N+1] -> dS f32[B,M+1,N+1] = dL/dS0 (exactly zero on masked rows / columns, whatever G
 * holds there; all zero for a problem without a valid row or column) and d_alpha_part f32[B] = the per-problem sum of dS over the dustbin
 * row and column.  The duals of all `iters` iterations are recomputed and recorded by the call itself (no early exit, no truncation).
 * Deterministic: no floating-point atomics, a problem's result does not depend on its batch.  Form 0 (M+1, N+1 <= 132): one resident
 * workgroup per problem; form 1: one launch per half-step.  The _ws_bytes and _form queries are host-only; B == 0 is a no-op returning 0;
 * a short workspace, iters < 1 or a null pointer is refused before any launch.  ws is written in full or in part and holds nothing on
 * return that a caller should read. */
int lcr_log_sinkhorn_grad_ws_bytes(int64_t B, int M, int N, int iters, size_t* bytes);
int lcr_log_sinkhorn_grad_form(int64_t B, int M, int N, int* form);
int lcr_log_sinkhorn_grad(const float* S0, const float* G, const uint8_t* row_mask, const uint8_t* col_mask, int64_t B, int M, int N,
                          int iters, float inf_val, float* dS, float* d_alpha_part, void* ws, size_t ws_bytes, void* stream);
/* Dustbin top-1 matching in the exp domain (superpoint_matching.py:130-162; local_global_registration.py:49-92 with k=1,
 * mutual=False, use_dustbin=True): (b,i,j) kept if it is its row's maximum beating the dustbin column OR its column's
 * maximum beating the dustbin row (and row/col masks, if given).  Phase 1: out_bij == NULL -> *total (device i64);
 * phase 2: same arguments with out_bij i32[total,3], out_score f32[total].  Row-major order. */
int lcr_top1_matching_ws_bytes(int64_t B, int M, int N, size_t* bytes);
int lcr_top1_matching(const float* logS, int64_t B, int M, int N, const uint8_t* row_mask, const uint8_t* col_mask,
                      int64_t* total, int32_t* out_bij, float* out_score, void* ws, size_t ws_bytes, void* stream);
/* Same with the `mutual` switch of LocalGlobalRegistration (local_global_registration.py:84-87): != 0 keeps a pair only if it is both
 * its row's and its column's maximum (each beating its dustbin); 0 = either, the shipped configuration. */
int lcr_top1_matching_ex(const float* logS, int64_t B, int M, int N, const uint8_t* row_mask, const uint8_t* col_mask, int mutual,
                         int64_t* total, int32_t* out_bij, float* out_score, void* ws, size_t ws_bytes, void* stream);
/* The patch score matrices of the dense point matching (model_family/LCRNet.py:236-250 + the padding of learnable_sinkhorn.py:38-49) in one
 * kernel: S[p] f32[(K+1),(K+1)] = scale * gather(feats_a, idx_a[p]) . gather(feats_b, idx_b[p])^T over C channels on the fp32 matrix cores,
 * dustbin row / column = *alpha, entries of masked rows / columns = -inf_val — what lcr_build_padded_scores makes of the batched product of
 * two lcr_gather_rows results, without the gathered copies.  idx_* i64[P,K] with the shadow index (== N*) for a zero row, mask_* u8[P,K];
 * K = 128 (cfg.model.num_points_in_patch), C % 32 == 0, feats 16-byte aligned.  feats_a / feats_b may be the same tensor. */
int lcr_patch_scores(const float* feats_a, int64_t Na, const float* feats_b, int64_t Nb, int C, const int64_t* idx_a, const int64_t* idx_b,
                     const uint8_t* mask_a, const uint8_t* mask_b, int64_t P, int K, float scale, const float* alpha, float inf_val, float* S,
                     void* stream);
/* Reverse pass of lcr_patch_scores with respect to the two feature tensors (csrc/patch_scores.hip).  dS f32[P,K+1,K+1] is what
 * lcr_log_sinkhorn_grad returns; feats / idx / mask / scale are the forward's.  G[p] = scale * dS[p][:K,:K] with every entry of a masked row or
 * column taken as zero BY SELECT (dS may hold anything there, NaN included); the dustbin row and column are never read (d_alpha stays with the
 * transport's d_alpha_part).  dA_g[p] = G[p] . gather(feats_b, idx_b[p]), dB_g[p] = G[p]^T . gather(feats_a, idx_a[p]) on the fp32 matrix cores,
 * contraction index ascending; d_feats_a f32[Na,C] row n = the sum of dA_g[p][i] over the slots with idx_a[p,i] == n in ascending p K + i,
 * d_feats_b likewise.  The shadow index (== N*) and any index outside [0, N*) receive nothing; a row nobody lists is exactly zero.  idx is
 * general: a row may be listed by several patches and several times by one.  (row_start_*, edges_*) = lcr_neighbor_transpose of idx_* viewed
 * as [P,K] over N* rows.  Either gradient may be NULL (its list is then not read).  No floating-point atomics, every output element written
 * once, results repeat to the bit and a patch's products do not depend on its batch.  Domain as the forward: K = 128, C % 32 == 0, features,
 * gradients and workspace 16-byte aligned, P * K < 2^30; LCR_EARG with text outside it.  P == 0 zero-fills the gradients.  ws:
 * lcr_patch_scores_grad_ws_bytes(P, K, C) = 2 P K C floats, host-only query (8 MB per pair and side at the training sizes P <= 128, C = 128:
 * not chunked). */
int lcr_patch_scores_grad_ws_bytes(int64_t P, int K, int C, size_t* bytes);
int lcr_patch_scores_grad(const float* dS, const float* feats_a, int64_t Na, const float* feats_b, int64_t Nb, int C, const int64_t* idx_a,
                          const int64_t* idx_b, const uint8_t* mask_a, const uint8_t* mask_b, int64_t P, int K, float scale,
                          const int32_t* row_start_a, const uint32_t* edges_a, const int32_t* row_start_b, const uint32_t* edges_b,
                          float* d_feats_a, float* d_feats_b, void* ws, size_t ws_bytes, void* stream);
/* Dustbin top-K matching for K >= 1 (LocalGlobalRegistration(k=K), local_global_registration.py:56-82; K = 1 in the shipped configuration):
 * (i, j) is kept from the row side if P[i][j] is among the K largest of row i — dustbin column included, equal values in index order — and
 * beats the row's dustbin; from the column side likewise; `mutual` as above.  Two-phase and row-major like lcr_top1_matching. */
int lcr_topk_matching_ws_bytes(int64_t B, int M, int N, size_t* bytes);
int lcr_topk_matching(const float* logS, int64_t B, int M, int N, const uint8_t* row_mask, const uint8_t* col_mask, int K, int mutual,
                      int64_t* total, int32_t* out_bij, float* out_score, void* ws, size_t ws_bytes, void* stream);
/* Every switch of LocalGlobalRegistration.compute_correspondence_matrix (local_global_registration.py:48-93):
 *   use_dustbin = 0 (:62-65, :74-77; LCRNet.py:256-257 strips the dustbin first): the K largest are taken over the M x N interior, the selected
 *     values are scattered into a zero matrix and kept where that exceeds `confidence_threshold` (an unselected entry counts as 0);
 *   global_scores f32[B] or NULL (use_global_score, :236-237): emitted scores of patch pair b are multiplied by global_scores[b].
 * logS is the (M+1) x (N+1) transport output in both forms.  use_dustbin = 1, threshold ignored, NULL = lcr_topk_matching. */
int lcr_topk_matching_ex(const float* logS, int64_t B, int M, int N, const uint8_t* row_mask, const uint8_t* col_mask, int K, int mutual,
                         int use_dustbin, float confidence_threshold, const float* global_scores, int64_t* total, int32_t* out_bij,
                         float* out_score, void* ws, size_t ws_bytes, void* stream);
/* out[n] = [ x[idx[n,0]] (zeros for the shadow index), skip[n] ]  (nearest_upsample + cat, backbone4.py:355-367) */
int lcr_upsample_concat(const float* x, int64_t Nx, int C1, const void* idx, int idx_is_64, int H, const float* skip, int C2,
                        int64_t N, float* out, void* stream);
/* Reverse passes of lcr_vote_shift, lcr_neighbor_mean and lcr_upsample_concat (csrc/pose_tail.hip), in the manner of the encoder's: gathers
 * over an inverted list (lcr_neighbor_transpose), every sum in one fixed order, no floating-point atomics, results repeat to the bit and
 * a cloud's rows get the same bytes alone and inside a stack.  LCR_EARG with text and no launch outside the domain; no rows: a no-op.
 *
 * lcr_vote_shift_grad: d_off [N,3] from g = d_out [N,3] (d_xyz = g needs no kernel).  |o| <= R: d_off = g; else, with a = R / |o| and
 * o^ = o / |o|, d_off = a (g - o^ (o^ . g)).  The branch is the forward's comparison (|o| > R) on the forward's own |o|.
 * lcr_neighbor_mean_grad: d_pts[j] = sum of d_out[m] / c_m over the edges (m,h) of j, c_m = the number of valid entries of row m counted
 * as the forward counts them; (row_start, edges) = the inverted form of idx [M,H] over `pad` points.  H <= 128, M * H < 2^30.
 * lcr_upsample_concat_grad: d_out [N, C1 + C2] -> d_x [Nx, C1] with d_x[j] = sum of d_out[n][:C1] over the rows n with idx[n,0] == j in
 * ascending n — (row_start, edges) = the inverted form of COLUMN 0 of idx as an [N,1] list over Nx rows; the shadow index sends its
 * gradient nowhere and a row nobody lists gets zeros — and d_skip [N, C2] = d_out[:, C1:].  Either output may be NULL (d_skip alone
 * needs no list).  N < 2^30. */
int lcr_vote_shift_grad(const float* offsets, const float* d_out, int64_t N, float max_range, float* d_off, void* stream);
int lcr_neighbor_mean_grad(const float* d_out, const void* idx, int idx_is_64, const int32_t* row_start, const uint32_t* edges, int64_t M,
                           int H, int64_t pad, float* d_pts, void* stream);
int lcr_upsample_concat_grad(const float* d_out, const int32_t* row_start, const uint32_t* edges, int64_t N, int64_t Nx, int C1, int C2,
                             float* d_x, float* d_skip, void* stream);
/* out[r] = src[idx[r]] (zeros where idx == pad): index_select on a zero-padded tensor */
int lcr_gather_rows(const float* src, int64_t pad, int C, const int64_t* idx, int64_t R, float* out, void* stream);
/* weighted_procrustes (modules/registration/procrustes.py:6-73), batched: problem p = correspondences [start[p],start[p+1]);
 * 3x3 SVD on the device (one-sided Jacobi, fp64); T f32[P,4,4].  An empty range or all-zero weights (H == 0) give the identity, as torch.svd
 * does; rank <= 1 inputs give some proper rotation of least residual. */
int lcr_procrustes_batched(const float* src, const float* ref, const float* w, const int32_t* start, int P, float eps, float* T, void* stream);
/* counts[p] = #{ |ref - T_p src| < radius } (-1 if the hypothesis came from < min_count correspondences); best = first argmax */
int lcr_inlier_count(const float* T, int P, const float* src, const float* ref, int n, float radius, const int32_t* start,
                     int min_count, int32_t* counts, int32_t* best, void* stream);
/* local_to_global_registration (geotransformer/local_global_registration.py:134-201) for S pairs in one launch sequence:
 * correspondences stacked pair-major; hypothesis h = weighted Procrustes of rows [hyp_start[h], hyp_start[h+1]) (one per patch
 * correspondence); pair s owns hypotheses [seg_hyp_start[s], seg_hyp_start[s+1]).  Per pair: inlier counts of its hypotheses over
 * its own rows (chunks below min_count rows never win), first argmax, then `steps` re-weighted refits; a pair without a valid
 * hypothesis starts from the fit over all its rows.  T_out f32[S,4,4]; optional hyp_out f32[H,4,4], counts_out i32[H], best_out
 * i32[S] (-1: fallback).  No host synchronisation. */
int lcr_lgr_ws_bytes(int64_t n, int H, int S, size_t* bytes);
int lcr_local_global_registration(const float* src, const float* ref, const float* score, int64_t n, const int32_t* hyp_start, int H,
                                  const int32_t* seg_hyp_start, int S, float radius, int min_count, int steps, float* T_out,
                                  float* hyp_out, int32_t* counts_out, int32_t* best_out, void* ws, size_t ws_bytes, void* stream);
/* Same with LocalGlobalRegistration(correspondence_limit=L) (:152-160): a pair with more than L correspondences verifies (inlier counts, the
 * degenerate-branch fit and every refit) on its L highest-scoring ones only — ties at the L-th score in row order — while the hypotheses
 * still come from all rows of their patch correspondence.  L = 0: no limit (= lcr_local_global_registration).  Same workspace size. */
int lcr_local_global_registration_ex(const float* src, const float* ref, const float* score, int64_t n, const int32_t* hyp_start, int H,
                                     const int32_t* seg_hyp_start, int S, float radius, int min_count, int steps, int correspondence_limit,
                                     float* T_out, float* hyp_out, int32_t* counts_out, int32_t* best_out, void* ws, size_t ws_bytes,
                                     void* stream);
/* w_out = score * [ |ref - T src| < radius ], T = T_all[sel ? *sel : 0]  (recompute_correspondence_scores, LGR :127-132) */
int lcr_inlier_weights(const float* T_all, const int32_t* sel, const float* src, const float* ref, const float* score, int n,
                       float radius, float* w_out, void* stream);

/* Correspondence RANSAC (utils/utils/open3d.py:145-173: Open3D's registration_ransac_based_on_correspondence, point-to-point without
 * scaling, RANSACConvergenceCriteria(N, N) so that every iteration runs), for S pairs in one call.  Open3D's sampling is random; this
 * one is deterministic and defined as follows.
 *   - Pairs: correspondences stacked pair-major, pair s = rows [start[s], start[s+1]) of src / ref f32[n,3] (n_s rows; start int32 [S+1]).
 *     The result maps src onto ref (experiments/registration/eval.py passes src = anchor, ref = positive).
 *   - Sampler: hypothesis h (0 <= h < iterations) draws ransac_n rows with replacement (as Open3D's RandUint32() % size does).  Draw j
 *     is z = SplitMix64(seed + 0x9E3779B97F4A7C15 * (1 + 8h + j)) (the finaliser: z ^= z >> 30, *= 0xBF58476D1CE4E5B9, ^= z >> 27,
 *     *= 0x94D049BB133111EB, ^= z >> 31; all mod 2^64), row = (hi32(z) * n_s) >> 32.  The key leaves the pair's position in the batch
 *     out: a pair gives bit-identical results alone or inside any batch.  lcr_ransac_sample_host computes the same indices on the host.
 *   - Hypothesis: Kabsch with unit weights on the sampled rows; centroids and H = sum (s - c_src)(r - c_ref)^T in fp64, R from the fp64
 *     Jacobi SVD of the weighted Procrustes (reflection fixed on the smallest singular direction), t = c_ref - R c_src, stored as fp32.
 *     INVALID (never selected) when the sample is coincident or collinear: sigma_2(H) <= 1e-9 sigma_1(H) or sigma_1(H) <= 1e-30.
 *   - Score, fp32: with m = the hypothesis' 12 floats (R|t row-major), dx = fma(m2, sz, fma(m1, sy, fma(m0, sx, m3))) - rx (dy, dz
 *     likewise), d2 = fma(dz, dz, fma(dy, dy, dx * dx)); row i is an inlier iff d2 < thr * thr (fp32 product).  Per hypothesis: inlier
 *     count and inlier SSE (sum of the inliers' d2 in row order, fp32).
 *   - Selection: most inliers, ties to the smaller SSE, then to the smaller h — a total order, so the result does not depend on launch
 *     order.  The winner's transform is returned as it is (no refit on its inliers), with its inlier count and RMSE = sqrt(SSE / count).
 *     A pair with n_s < ransac_n, without a valid hypothesis, or whose best hypothesis has no inlier returns the identity, 0 inliers,
 *     RMSE 0 and best_h -1 (Open3D returns an empty result there).
 * Outputs: T f32[S,4,4], inliers i32[S], rmse f32[S]; nullable: best_h i32[S], and the per-hypothesis detail T_all f32[S*iterations,4,4]
 * (the identity for invalid hypotheses), counts_all i32[S*iterations] (-1 = invalid), sse_all f32[S*iterations] (index s*iterations+h).
 * Three launches, no host synchronisation; ws: lcr_ransac_ws_bytes (~64 B per hypothesis).
 * Domain: 1 <= S <= 65535, 3 <= ransac_n <= 8, 1 <= iterations <= 1e6, any n_s >= 0, 0 < thr with thr * thr finite; LCR_EARG outside. */
int lcr_ransac_ws_bytes(int S, int iterations, size_t* bytes);
int lcr_ransac_correspondences(const float* src, const float* ref, const int32_t* start, int S, float thr, int ransac_n, int iterations,
                               uint64_t seed, float* T, int32_t* inliers, float* rmse, int32_t* best_h, float* T_all, int32_t* counts_all,
                               float* sse_all, void* ws, size_t ws_bytes, void* stream);
/* The sampler on the host: idx_host[k * ransac_n + j] = draw j of hypothesis h0 + k for a pair of n rows (1 <= n <= 2^31 - 1,
 * 1 <= ransac_n <= 8, 0 <= h0, h0 + count <= 1e6). */
int lcr_ransac_sample_host(uint64_t seed, int64_t h0, int64_t count, int ransac_n, int64_t n, int32_t* idx_host);
/* Correspondence RANSAC with Open3D's correspondence checkers (utils/utils/open3d.py:109-142 passes
 * CorrespondenceCheckerBasedOnEdgeLength(0.9) and CorrespondenceCheckerBasedOnDistance(distance_threshold)).  Sampler, hypothesis, score
 * and selection are those of lcr_ransac_correspondences (one code path: that entry is this one with both checks off and no corr, and
 * returns the same bits); a hypothesis that fails a check is INVALID exactly like a collinear sample: never selected, counts_all = -1,
 * sse_all = 0, the identity in T_all.
 *   - edge_similarity (<= 0: off), before the fit: for every two draws a < b of the sample, on the fp32 rows, ls2 = |s_a - s_b|^2 and
 *     lr2 = |r_a - r_b|^2 in the exact fp32 form (dx*dx + dy*dy) + dz*dz (every operation rounded), k2 = edge_similarity *
 *     edge_similarity (fp32 product); the sample passes iff ls2 >= k2 * lr2 and lr2 >= k2 * ls2 (fp32 products) for all of them.
 *     Squared lengths on purpose: no square root enters the definition.  A sample that fails is not fitted.
 *   - checker_distance (<= 0: off), after the fit: every sampled row must satisfy the scoring rule's own d2 < checker_distance *
 *     checker_distance (the fma form above on the stored fp32 transform, fp32 product on the right).
 *   - reject_all (nullable) uint8 [S*iterations]: 0 valid, 1 degenerate (collinear or coincident sample, or n_s < ransac_n), 2 edge check,
 *     3 distance check; the first check that fires in the order edge, degenerate, distance names the code.
 *   - With a check on, the surviving hypotheses of every pair are listed in ascending h (a fourth launch, one workgroup per pair) and
 *     the scoring pass runs over that list only: a rejected hypothesis streams no correspondence.  Selection's tie-break on h and the
 *     index s*iterations+h of the per-hypothesis outputs are those of the original h.
 *   - Index form: corr int32 [n_corr,2] non-null (pair-local src row, ref row; start [S+1] then offsets the rows of corr, and n_corr >=
 *     start[S] is the capacity of corr): src / ref are the pairs' point clouds, stacked pair-major with src_start / ref_start int32 [S+1].
 *     The rows are gathered by a kernel of its own into the workspace (12 B per row and side) and the rest of the call sees the layout of
 *     lcr_ransac_correspondences, so the two forms give the same bits.  An index outside its cloud yields a NaN row (never an inlier).
 *     corr null: src / ref are the correspondence rows themselves; src_start, ref_start and n_corr are not read.
 * ws: lcr_ransac_ex_ws_bytes(S, iterations, n_corr) (n_corr = 0 without corr).  Domain: that of lcr_ransac_correspondences, the squares
 * of the two checker parameters finite, 0 <= n_corr <= 2^31-1; LCR_EARG outside. */
int lcr_ransac_ex_ws_bytes(int S, int iterations, int64_t n_corr, size_t* bytes);
int lcr_ransac_correspondences_ex(const float* src, const float* ref, const int32_t* start, int S, const int32_t* corr, const int32_t* src_start,
                                  const int32_t* ref_start, int64_t n_corr, float thr, int ransac_n, int iterations, uint64_t seed,
                                  float edge_similarity, float checker_distance, float* T, int32_t* inliers, float* rmse, int32_t* best_h,
                                  float* T_all, int32_t* counts_all, float* sse_all, uint8_t* reject_all, void* ws, size_t ws_bytes, void* stream);

/* Exact nearest neighbour in feature space (what Open3D's registration_ransac_based_on_feature_matching asks of a KD-tree over the
 * features), for S pairs in one call.
 *   - Pairs: queries qf f32[nq,C] and database df f32[nd,C] stacked pair-major; pair s = query rows [q_start[s], q_start[s+1]) and
 *     database rows [d_start[s], d_start[s+1]) (int32 [S+1] on the device).  A query only sees the database of its own pair.
 *   - d2(i, j), fp32 with every operation rounded (no contraction): acc = 0; for c = 0 .. C-1: t = q[c] - d[c]; acc = acc + t * t.
 *   - nn(i) = the pair-local database row j that minimises (d2(i, j), j) lexicographically: ties go to the smaller row.  A total order,
 *     so the result depends on no tile, slice or launch order, and a pair gives the same bits alone or in any batch.
 *   - Non-finite features: a NaN distance never wins (+inf is an ordinary value and can).  A row whose every distance is NaN, and every
 *     row of a pair with an empty database, gets nn = -1 and d2 = NaN (0x7fc00000).
 *   - Outputs per query row: nn int32 [nq], d2 f32 [nq] (the minimum itself).
 *   - Every (i, j) is evaluated by the chain above on the vector unit (no screening pass, so nothing rests on an error bound):
 *     3 nq nd C rounded operations.  Three stream-ordered launches and a scan over the pairs, no host synchronisation, no allocation; the workspace holds one
 *     (d2, row) per query and database slice (at most 16 slices), never an nq x nd matrix.
 * Domain: 1 <= S <= 65535, 1 <= C <= 1024, 0 <= nq, nd <= 2^31-1 (the row counts of qf / df); LCR_EARG outside. */
int lcr_feature_nn_ws_bytes(int S, int64_t nq, int64_t nd, size_t* bytes);
int lcr_feature_nn(const float* qf, const float* df, const int32_t* q_start, const int32_t* d_start, int S, int C, int64_t nq, int64_t nd,
                   int32_t* nn, float* d2, void* ws, size_t ws_bytes, void* stream);
/* Correspondences from nearest-neighbour rows, per pair: the rows (i, nn_sr[i]) in ascending i (both pair-local), keeping i iff
 * 0 <= nn_sr[i] < the pair's ref rows and (nn_rs null, or nn_rs[nn_sr[i]] == i: the mutual filter).  As Open3D does, a pair whose mutual
 * set has fewer than min_rows (= ransac_n) rows falls back to its unfiltered set, decided on the device.  nn_sr int32 [ns] stacked with
 * src_start [S+1], nn_rs int32 [nr] stacked with ref_start [S+1].  Outputs: corr int32 [ns,2] (capacity: one row per source row; the first
 * start[S] are written), start int32 [S+1] (exclusive scan of the pairs' counts), nullable mutual_used int32 [S] (1 where the filter held).
 * Ordered compaction by wavefront ballot and prefix, no atomics; three launches and a scan, no host synchronisation.
 * Domain: 1 <= S <= 65535, min_rows >= 0; LCR_EARG outside. */
int lcr_feature_correspondences_ws_bytes(int S, size_t* bytes);
int lcr_feature_correspondences(const int32_t* nn_sr, const int32_t* src_start, const int32_t* nn_rs, const int32_t* ref_start, int S, int min_rows,
                                int32_t* corr, int32_t* start, int32_t* mutual_used, void* ws, size_t ws_bytes, void* stream);

/* Ground-truth node correspondences (patch overlaps) under the ground-truth transform, for P pairs in one call: the labels behind the
 * coarse-matching metrics (reference: modules/registration/matching.py:252-349, one pair at a time in torch).
 *   - Inputs: what lcr_point_to_node_partition_stack emits for the 2P clouds [pos_0, anc_0, pos_1, anc_1, ...]: points f32[sum N,3] with
 *     HOST point_off i64[2P+1], nodes f32[sum M,3] with HOST node_off i64[2P+1] (rows point_off[c] .. of points and node_off[c] .. of
 *     nodes belong to cloud c; knn and the masks start at the first cloud's first node), knn i64[sum M,K] cloud-local, knn_mask
 *     u8[sum M,K], node_mask u8[sum M]; transforms f32[P,16] on the device, row-major 4x4, anc (src) onto pos (ref).  The node centres
 *     are not read: the definition has no use for them.
 *   - A patch entry (node, k) is valid iff node_mask[node] and knn_mask[node,k] are set and 0 <= knn[node,k] < the cloud's point count.
 *   - r2 = (float)(pos_radius * pos_radius).  Each anc point (x, y, z) is moved once: q' = ((R0*x + R1*y) + R2*z) + t per component
 *     (R0 R1 R2 t = that row of the 4x4), every operation fp32 and rounded, no contraction.
 *   - A point pair (p of the ref patch, q' of the src patch) is NEAR iff ((dx*dx + dy*dy) + dz*dz) < r2 with d = p - q', fp32, every
 *     operation rounded, the comparison strict.  A non-finite coordinate is therefore never near.
 *   - For ref node i (pos) and src node j (anc): cr = valid points of patch i near at least one valid point of patch j, cs = the converse,
 *     nr / ns = the valid counts.  (i, j) is a correspondence iff cr > 0 (equivalently cs > 0);
 *     overlap = ((float)cr / (float)nr + (float)cs / (float)ns) / 2 with IEEE fp32 divisions.  A node without a valid point never appears.
 *   - The reference's enclosing-sphere screen (matching.py:311-321) is NOT part of the definition; the screen used here (axis-aligned boxes
 *     of the valid finite points, tested with a radius whose rounded square is >= r2) cannot drop a near pair.  The reference decides
 *     nearness on |x|^2 - 2 x.y + |y|^2, whose rounding at 80 m coordinates is of the order of r2's last digits: DESIGN.md section 8.
 *   - Outputs: corr i32[cap,2] pair-local (ref node, src node), row-major within a pair, pairs in order; overlap f32[cap]; start i32[P+1],
 *     the exclusive scan of the pairs' counts; status u32[1], written (not or-ed): LCR_STATUS_CAP_EXCEEDED iff start[P] > cap, else 0.
 *     start always holds the true counts; rows at or beyond cap are not written.  cap = sum M_p * N_p can never overflow.
 *   - Stream-ordered launches only (six and a scan), no host synchronisation, no allocation, no atomics; ordered compaction by wavefront
 *     ballot and prefix.  A pair gives the same bytes alone or in any batch.
 * Domain: 1 <= P <= 32, 1 <= K <= 2048, non-decreasing offsets, at most 2^31-1 points, nodes and sum M_p * N_p, cap >= 0, pos_radius >= 0
 * with a finite fp32 square; empty clouds and empty node lists are legal and give zero rows.  LCR_EARG outside.  The partition itself
 * takes any K >= 1; a patch wider than 2048 points does not fit the wavefront's LDS. */
#define LCR_STATUS_CAP_EXCEEDED 4u
int lcr_node_correspondences_ws_bytes(const int64_t* point_off, const int64_t* node_off, int P, int K, size_t* bytes);
int lcr_node_correspondences(const float* points, const int64_t* point_off, const float* nodes, const int64_t* node_off, const int64_t* knn,
                             const uint8_t* knn_mask, const uint8_t* node_mask, const float* transforms, int P, int K, double pos_radius,
                             int64_t cap, int32_t* corr, float* overlap, int32_t* start, uint32_t* status, void* ws, size_t ws_bytes,
                             void* stream);

/* Point-to-point ICP (Open3D's RegistrationICP with TransformationEstimationPointToPoint(with_scaling=False), as the reference's pair
 * generators run it: data/Kitti/generate_kitti_pairs.py:145-147) for S pairs in one call, made exact and batch-invariant.
 *   - Pairs: source rows stacked pair-major in src f32[ns,3], target rows in tgt f32[nt,3]; src_len / tgt_len are HOST int64[S].
 *     init f64[S,4,4] maps source onto target.  Coordinates must be finite (the domain; not checked on the device).
 *   - Correspondence step at pose T (fp64): source row i (x, y, z) becomes q = fp32(((T00*x + T01*y) + T02*z) + T03) (likewise y, z; no
 *     contraction).  Its partner is the target row of the same pair with the smallest (d2, row) among those with d2 < r*r (fp32 product),
 *     d2 = ((dx*dx)+dy*dy)+dz*dz in fp32 without FMA: the row lcr_radius_query_ordered(..., limit = 1) returns for q.
 *     count = partnered rows, fitness = count / n_src, inlier_rmse = sqrt(sum d2 / count) with the sum in fp64 (0 when count = 0).
 *   - Update: unit-weight Kabsch on the ORIGINAL source rows p_i and their partners r_j: fp64 centroids and H (moments accumulated
 *     about the first source / target row of the pair), R from the fp64 Jacobi SVD (reflection fixed on the smallest singular
 *     direction), T <- [R | c_r - R c_p] (equal to Open3D's update * T in exact arithmetic).  T is left unchanged when count < 3 or
 *     H is degenerate (sigma_2 <= 1e-9 sigma_1 or sigma_1 <= 1e-30).
 *   - Loop (Registration.cpp): result_0 at init; for k = 0 .. max_iteration-1: update, result_{k+1}; stop when
 *     |fitness_{k+1} - fitness_k| < relative_fitness AND |rmse_{k+1} - rmse_k| < relative_rmse.  iterations = updates performed.
 *   - Outputs at the final T: T f64[S,4,4], fitness f64[S], inlier_rmse f64[S], iterations i32[S].  Nullable: corr i32[ns] (pair-local
 *     target row of every source row at the final T, or -1), T_hist f64[S, max_iteration+1, 4, 4], fitness_hist / rmse_hist
 *     f64[S, max_iteration+1] (row k = T_k and result_k for k <= iterations; later rows are not written).
 *   - A pair with an empty source or target returns init, fitness 0, rmse 0, iterations 0; max_iteration = 0 returns init with result_0.
 *   - Determinism: every reduction is a fixed tree over the pair's own rows (no float atomics): a pair gives bit-identical outputs alone
 *     or at any position in any batch, and for any check_every.
 *   - Host loop: per iteration two launches; every check_every iterations one 4-byte read-back and a stream synchronisation, stopping
 *     once no pair runs; check_every = 0 never synchronises (all max_iteration trips; finished pairs are no-ops).  No allocation;
 *     ws: lcr_icp_ws_bytes(S, ns, nt).
 * Domain: 1 <= S <= 64, 0 <= max_iteration <= 100000, 0 < r with r*r finite, relative criteria >= 0, check_every >= 0, ns, nt <= 2^31-1;
 * LCR_EARG outside. */
int lcr_icp_ws_bytes(int S, int64_t ns, int64_t nt, size_t* bytes);
int lcr_icp_point_to_point(const float* src, const int64_t* src_len, const float* tgt, const int64_t* tgt_len, int S, const double* init,
                           float max_correspondence_distance, int max_iteration, double relative_fitness, double relative_rmse, double* T,
                           double* fitness, double* inlier_rmse, int32_t* iterations, int32_t* corr, double* T_hist, double* fitness_hist,
                           double* rmse_hist, int check_every, void* ws, size_t ws_bytes, void* stream);

/* Point-to-plane ICP (Open3D's RegistrationICP with TransformationEstimationPointToPlane(), no robust kernel): the arguments, outputs,
 * loop, stopping rule, check_every, history, determinism and domain of lcr_icp_point_to_point, plus tgt_normals f32[nt,3] (stacked like
 * tgt; lcr_estimate_normals writes them).
 *   - Correspondence step: unchanged (the same q, partner, count, fitness, inlier_rmse and corr rows as point-to-point at any pose).
 *   - Update: every partnered source row i whose partner j has a non-zero normal is usable.  s = T p_i in fp64 (((T00*x + T01*y) +
 *     T02*z) + T03, not the rounded q), t = tgt_j, n = normal_j, r = ((s-t)_x n_x + (s-t)_y n_y) + (s-t)_z n_z, J = [s x n, n].
 *     A = sum J J^T (21 unique entries) and g = sum J r in fp64, over the same fixed tree of the pair's rows as point-to-point.
 *     A x = -g is solved by fp64 LDL^T without pivoting; dT = [Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)] (Open3D's
 *     TransformVector6dToMatrix4d, linearised about the target frame's origin) and T <- dT T.  T is left unchanged when fewer than 6
 *     rows are usable or a pivot is <= 1e-12 times the largest diagonal entry of A (all usable rows on one plane, for example).
 *   - Partners with a zero normal count for fitness and inlier_rmse, and stay out of A and g.
 *   - ws: lcr_icp_plane_ws_bytes(S, ns, nt) (30 doubles per block row against point-to-point's 17; lcr_icp_ws_bytes does not cover it). */
int lcr_icp_plane_ws_bytes(int S, int64_t ns, int64_t nt, size_t* bytes);
int lcr_icp_point_to_plane(const float* src, const int64_t* src_len, const float* tgt, const int64_t* tgt_len, const float* tgt_normals, int S,
                           const double* init, float max_correspondence_distance, int max_iteration, double relative_fitness,
                           double relative_rmse, double* T, double* fitness, double* inlier_rmse, int32_t* iterations, int32_t* corr,
                           double* T_hist, double* fitness_hist, double* rmse_hist, int check_every, void* ws, size_t ws_bytes, void* stream);

/* Generalized ICP (plane-to-plane; Open3D's registration_generalized_icp with TransformationEstimationForGeneralizedICP(epsilon), no
 * robust kernel): the arguments, outputs, loop, stopping rule, check_every, history, determinism and domain of lcr_icp_point_to_plane,
 * plus src_normals f32[ns,3] (stacked like src; lcr_estimate_normals writes them) and epsilon.
 *   - Correspondence step: unchanged (the same q, partner, count, fitness, inlier_rmse (Euclidean, as Open3D's RegistrationICP loop uses
 *     for every estimator) and corr rows as point-to-point at any pose).
 *   - Covariance of a row with normal n (fp32 promoted to fp64, not renormalised): C(n) = I - (1 - epsilon) n n^T, the surface model
 *     "epsilon along the normal, 1 across it" (R diag(epsilon, 1, 1) R^T for a unit n).  A zero normal (a degenerate row of
 *     lcr_estimate_normals) gives C = I.
 *   - Update at pose T (rows 0..2, Rm = its 3x3) over every partnered source row i with partner j: s = T p_i in fp64 (((T00*x + T01*y) +
 *     T02*z) + T03, not the rounded q), t = tgt_j, d = s - t, a = Rm n_i with the same association ((Tr0*nx + Tr1*ny) + Tr2*nz),
 *     b = n_j, M = 2I - (1 - epsilon)(a a^T + b b^T) (= C_t + Rm C_s Rm^T), W = M^-1 in fp64 (symmetric 3x3, adjugate / determinant),
 *     J = [-[s]x | I] (3x6).  A = sum J^T W J (21 unique entries) and g = sum J^T W d in fp64, over the same fixed tree of the pair's
 *     rows as the other two estimators.  A x = -g is solved by the LDL^T of point-to-plane with its pivot rule, and T <- dT(x) T with the
 *     same dT (Open3D's TransformVector6dToMatrix4d).  T is left unchanged when count < 3 or a pivot fails.
 *   - Relation to Open3D: its GICP builds per-point covariances R diag(epsilon, 1, 1) R^T from a normal, or from the estimated
 *     covariance with its eigenvalues replaced by (epsilon, 1, 1), the normal being the smallest eigenvector; C(n) above is that matrix.
 *     Parity with Open3D's binary is not pinned (as for lcr_estimate_normals and lcr_fpfh); tests/gicp_restatement.py is the definition.
 *   - ws: lcr_icp_generalized_ws_bytes(S, ns, nt).  The call uses 29 doubles per block row (count, sum d2, A[21], g[6]); the query never
 *     answers less than lcr_icp_plane_ws_bytes, so a workspace of this size serves all three estimators on the same shapes.
 * Domain: that of lcr_icp_point_to_plane, plus 1e-6 <= epsilon <= 1 and non-null src_normals / tgt_normals where the side has rows.  The
 * lower bound keeps M positive definite when two fp32-rounded unit normals are parallel (its smallest eigenvalue is then
 * 2 epsilon - O(1e-7)); normals are expected to be unit or zero.  LCR_EARG outside. */
int lcr_icp_generalized_ws_bytes(int S, int64_t ns, int64_t nt, size_t* bytes);
int lcr_icp_generalized(const float* src, const int64_t* src_len, const float* src_normals, const float* tgt, const int64_t* tgt_len,
                        const float* tgt_normals, int S, const double* init, float max_correspondence_distance, double epsilon,
                        int max_iteration, double relative_fitness, double relative_rmse, double* T, double* fitness, double* inlier_rmse,
                        int32_t* iterations, int32_t* corr, double* T_hist, double* fitness_hist, double* rmse_hist, int check_every,
                        void* ws, size_t ws_bytes, void* stream);

/* Surface normals (Open3D's EstimateNormals with KDTreeSearchParamHybrid(radius, max_nn), as utils/utils/open3d.py:53-58 calls it) for B
 * stacked clouds in one call, made exact and batch-invariant.
 *   - Input: points f32[N,3] stacked cloud-major, lengths HOST int64[B]; radius > 0; 1 <= max_nn <= 128; viewpoint f32[B,3] on the
 *     device or NULL (the origin of every cloud's frame: the sensor).  Coordinates must be finite (not checked on the device).
 *   - Neighbourhood of row i: the rows j of the same cloud with d2 < radius*radius (fp32 product), d2 = ((dx*dx)+dy*dy)+dz*dz in fp32
 *     without FMA; of these the max_nn with the smallest (d2, row), row i itself included: the first max_nn rows
 *     lcr_radius_query_ordered(q = s = the cloud, limit = max_nn) returns for i.  k = their number.
 *   - Covariance in fp64 about the query point p_i: d = p_j - p_i per selected row, s_a = sum d_a, s_ab = sum d_a d_b (summed in
 *     ascending row order), c_ab = s_ab / k - (s_a / k) (s_b / k): Open3D's ComputeCovariance in exact arithmetic.
 *   - Normal: the unit eigenvector of the smallest eigenvalue lam0 <= lam1 <= lam2 (fp64 Jacobi), oriented so that n . (v - p_i) >= 0
 *     (fp64); where that product is exactly 0, the first non-zero component of n is made positive.
 *   - Degenerate rows (k < 3, lam2 <= 1e-30, or lam1 <= 1e-12 lam2: coincident or collinear neighbours) get the zero normal.
 *   - Outputs: normals f32[N,3]; nullable curvature f32[N] (lam0 / (lam0 + lam1 + lam2), 0 for degenerate rows) and count i32[N] (k).
 *   - Determinism: a cloud gives bit-identical outputs alone or at any position in any batch.
 *   - Asynchronous and stream-ordered, no allocation; ws: lcr_normals_ws_bytes(B, N).
 * Domain: 1 <= B <= 64, 0 < radius with radius*radius finite, 1 <= max_nn <= 128, lengths >= 0, N <= 2^31-1; LCR_EARG outside. */
int lcr_normals_ws_bytes(int B, int64_t n, size_t* bytes);
int lcr_estimate_normals(const float* points, const int64_t* lengths, int B, float radius, int max_nn, const float* viewpoint, float* normals,
                         float* curvature, int32_t* count, void* ws, size_t ws_bytes, void* stream);

/* FPFH descriptors (Open3D's compute_fpfh_feature with KDTreeSearchParamHybrid(radius, max_nn): the 33-bin hand-crafted feature that
 * registration_ransac_based_on_feature_matching is documented with) for B stacked clouds in one call, from the points and normals alone.
 *   - Input: points f32[N,3] and normals f32[N,3] stacked cloud-major (lcr_estimate_normals writes such normals), lengths HOST int64[B].
 *   - Neighbourhood of row i: the first max_nn rows lcr_radius_query_ordered(q = s = the cloud, limit = max_nn) returns for i, that is
 *     the rows of the same cloud with d2 < radius*radius (fp32 product), d2 = ((dx*dx)+dy*dy)+dz*dz in fp32 without FMA, ascending by
 *     (d2, row); row i itself is then removed from that list WHEREVER it stands.  Open3D drops the first entry, which is the row itself
 *     unless the cloud has coincident points, where its choice depends on the KD-tree's order: this is the one place where the
 *     definition is made canonical.  m = the number of remaining rows; count = m.  m == 0 gives an all-zero feature and SPFH row.
 *   - Pair features, all arithmetic in fp64 on the fp32 inputs promoted, (p1, n1) = row i and (p2, n2) = the neighbour:
 *       dp = p2 - p1, d = |dp|; d == 0: f = (0, 0, 0).
 *       a1 = n1.dp / d, a2 = n2.dp / d.  Swap iff |a1| < |a2|; on a swap n1 <-> n2, dp = -dp, f2 = -a2; otherwise f2 = a1.
 *       (Open3D writes the swap as acos(|a1|) > acos(|a2|); the two agree whenever both cosines are <= 1.  An fp32-rounded normal can
 *       push a cosine past 1, where Open3D compares with a NaN: comparing the cosines is a deliberate canonical choice.)
 *       v = dp x n1; |v| == 0: f = (0, 0, 0).  Otherwise v /= |v|, w = n1 x v, f1 = v.n2, f0 = atan2(w.n2, n1.n2).
 *   - Bins: b0 = floor(11 (f0 + pi) / (2 pi)), b1 = floor(11 (f1 + 1) / 2), b2 = floor(11 (f2 + 1) / 2), each clamped to 0..10.  A
 *     zero-feature pair still votes, as in Open3D: bin 5 of each block (coincident points, zero (degenerate) normals).
 *   - SPFH: spfh(i, 11 k + b_k) = (votes * 100) / m in fp64, one rounding.  The votes are integers: SPFH depends on no summation order.
 *   - FPFH: over the same list in its order, skipping neighbours with d2 == 0: acc_j = sum spfh(nb, j) / d2(nb), d2 the search's fp32
 *     value promoted, every division and sum rounded in fp64, in list order (which depends on the row's own list alone).  Per block of
 *     11: s = sum acc_j (ascending j); feature_j = acc_j * (s != 0 ? 100 / s : 0) + spfh(i, j), written rounded to fp32.
 *   - Outputs: features f32[N,33]; nullable spfh f32[N,33] (SPFH rounded to fp32) and count i32[N] (m).
 *   - Determinism: a cloud gives bit-identical outputs alone or at any position in any batch.  No float atomics.
 *   - Asynchronous and stream-ordered, no allocation, no host synchronisation; ws: lcr_fpfh_ws_bytes(B, N, max_nn) (the support grid, the
 *     int32 [N, max_nn] neighbour table and the fp64 SPFH rows).  The argument checks and lcr_fpfh_ws_bytes are host-only.
 * Parity against Open3D's own binary is unpinned; tests/fpfh_restatement.py restates exactly the text above.
 * Domain: 1 <= B <= 64, 0 < radius with radius*radius finite, 2 <= max_nn <= 128, lengths >= 0, N <= 2^31-1; LCR_EARG outside. */
int lcr_fpfh_ws_bytes(int B, int64_t n, int max_nn, size_t* bytes);
int lcr_fpfh(const float* points, const float* normals, const int64_t* lengths, int B, float radius, int max_nn, float* features, float* spfh,
             int32_t* count, void* ws, size_t ws_bytes, void* stream);

/* Range-image scan overlap: the labels "frame j overlaps frame i by more than 0.3" of the loop-detection evaluation, for B stacked scans
 * and P pairs of them per call.  The kernels emit integers only; the ratio is taken by the caller.
 *   Parameters (defaults of a 64-beam sensor): H = 64, W = 900, fov_up = 3 (degrees), fov_down = -25 (degrees), max_range = 50, eps = 1.
 *   Derived angles: fu = fov_up*pi/180, fd = fov_down*pi/180, fov = |fu| + |fd|.
 *   Projection of one point: (x, y, z) is fp32 and promoted to fp64.  The rigid transform M is f64[3,4], applied in fp64 with every
 *   operation rounded, no FMA, in this order: x' = ((M00*x + M01*y) + M02*z) + M03, and likewise for y' and z'.
 *     - d = sqrt((x'x' + y'y') + z'z').
 *     - The point is kept iff 0 < d < max_range.
 *     - yaw = -atan2(y', x').
 *     - pitch = asin(clamp(z'/d, -1, 1)).
 *     - u = 0.5*(yaw/pi + 1)*W.
 *     - v = (1 - (pitch + |fd|)/fov)*H.
 *     - Column = floor(u) clamped to 0..W-1.
 *     - Row = floor(v) clamped to 0..H-1.
 *     - Points outside the vertical field of view therefore land in the edge rows.
 *   Range image: a pixel holds the minimum over its points of d rounded to fp32.  Rounding is monotone, so this equals the minimum of
 *   the rounded values.  An empty pixel holds -1.
 *
 * lcr_range_images: points f32[N,3] stacked cloud-major, lengths HOST int64[B] -> images f32[B,H,W] with M = identity (applied like any
 * M, so a negative zero coordinate comes out as +0), and valid i32[B], the count of non-empty pixels.
 *
 * lcr_scan_overlap: for each of P pairs (i, j) = pairs[p] (device i32[P,2]) with rel[p] (device f64[P,3,4]; the caller passes
 * rel = inv(T_i)*T_j, computed on the host in fp64): cloud j is projected through rel[p] into a scratch image, which is compared with
 * images[i] (as lcr_range_images wrote it, with valid).  counts i32[P,3] =
 *     matches   the number of pixels non-empty in both images with |double(a) - double(b)| < eps,
 *     valid_cur = valid[i],
 *     valid_ref the number of non-empty pixels of the projected image.
 *   i == j is allowed.  A pair with an index outside 0..B-1 reads nothing, gets counts (-1, -1, -1) and raises status i32[1] (device) to
 *   the largest such p + 1; status is 0 after a call without one.
 *   - Determinism: the only atomics are integer ones (an integer minimum on the fp32 bit pattern of a positive depth is order-free).  A
 *     pair gives the same bytes alone or at any position in any call.  No float atomics.
 *   - Both entries are asynchronous and stream-ordered, no allocation, no host synchronisation; ws: lcr_range_images_ws_bytes(B) /
 *     lcr_scan_overlap_ws_bytes(B, P) (the clouds' prefix offsets: the images being built live in LDS, in bands of rows).  The argument
 *     checks and the _ws_bytes helpers are host-only.  P == 0 returns LCR_OK before every other check and launches nothing (status is
 *     then not written).
 * The definition is restated in tests/scan_overlap_restatement.py and is not pinned against the script that produced the reference's
 * seq-00 labels.
 * Domain: 1 <= B <= 64, 0 <= P <= 2^31-1, 1 <= H <= 128, 1 <= W <= 4096, 0 < max_range, 0 < eps, fov > 0 and finite, lengths >= 0,
 * N <= 2^31-1; LCR_EARG outside. */
int lcr_range_images_ws_bytes(int B, size_t* bytes);
int lcr_range_images(const float* points, const int64_t* lengths, int B, int H, int W, double fov_up, double fov_down, double max_range,
                     float* images, int32_t* valid, void* ws, size_t ws_bytes, void* stream);
int lcr_scan_overlap_ws_bytes(int B, int64_t P, size_t* bytes);
int lcr_scan_overlap(const float* points, const int64_t* lengths, int B, const float* images, const int32_t* valid, const int32_t* pairs,
                     const double* rel, int64_t P, int H, int W, double fov_up, double fov_down, double max_range, double eps, int32_t* counts,
                     int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* Registration loss terms (the reference's experiments/lcrnet/loss_reg.py: gap :96-159, node_gap :163-231, SingleSideChamferLoss_Brute
 * :21-45, VoteLoss_new :48-92) with the gradients a training step needs: to the scores and to the shifted nodes.  Restated in
 * tests/losses_restatement.py.
 *
 * lcr_gap_loss: B score slices grouped into P pairs.  Slice b is S[soff[b] ...], (n_b+1) x (m_b+1) row-major fp32 log-transport scores,
 * the last row and column being the dustbin; n_b = roff[b+1]-roff[b], m_b = coff[b+1]-coff[b]; row i of slice b is entry roff[b]+i of
 * every per-row table (p_pts, pmask, the first `rows` line statistics), column j entry coff[b]+j of every per-column table (q_pts, qmask,
 * the line statistics from `rows` on).  soff / roff / coff are DEVICE i64[B+1]; seg_start is DEVICE i32[P+1], pair p owning slices
 * seg_start[p] .. seg_start[p+1]-1.  The host passes the extents it allocated for: n_max, m_max, elems (S and labels), rows, cols.  A slice
 * or segment that does not fit them is skipped by every kernel and raises LCR_STATUS_LEN_MISMATCH: nothing outside the extents is touched.
 *   - Labels, two bits per score (bit 0 positive, bit 1 negative), for the inner (i < n, j < m) entries from one of two sources:
 *     LCR_GAP_LABELS_POINTS: q' = ((R0*x + R1*y) + R2*z) + t per component with the pair's row-major 4x4 (transforms f32[P,16]),
 *       d = p - q', d2 = ((dx*dx + dy*dy) + dz*dz), fp32, every operation rounded.  positive iff d2 < (float)(r*r) and pmask[i] and
 *       qmask[j]; negative iff d2 > (float)((2r)*(2r)), whatever the masks say (the reference does not mask its negatives).
 *     LCR_GAP_LABELS_OVERLAPS: corr i64[C,2] pair-local (i, j) with overlaps f32[C], pair p's entries being corr_start[p] ..
 *       corr_start[p+1]-1 (DEVICE i32[P+1]; c_max = the host's bound on a pair's count), written into the pair's FIRST slice.  An entry is
 *       positive iff overlap > (float)positive_overlap and both masks, negative iff its overlap is exactly 0; a node pair that is not
 *       listed is negative.  A pair's entries must be distinct node pairs; an index outside the slice is skipped and raises
 *       LCR_STATUS_INDEX_RANGE.
 *   - A line is a row i < n of a slice (candidates j = 0..m, the dustbin column included) or a column j < m (candidates i = 0..n).  Its
 *     dustbin entry is positive iff the line has no inner positive, else negative.  pos = the mean of -S over the line's positives
 *     (count >= 1); hinge = the sum over the line's NEGATIVES of max(pos + S + gamma, 0), an argument >= 0 counting as active; every
 *     other entry stands for the reference's constant 1e12 and contributes nothing.  fp64 on the fp32 scores.
 *   - A line is dropped iff (float)pos == 1e12f exactly (the reference's own test: the padded lines, whose dustbin score is -1e12).
 *   - Per pair: terms f32[P,3] = (mean over kept rows of log(hinge + 1), the same over kept columns, their mean), NaN where a pair keeps
 *     no line; kept i32[P,2].  Saved for the gradient: labels u8[elems] (the dustbin entries hold their line's dustbin label, the corner
 *     0); line_pos f64, line_hinge f64, line_count i32 (positives), line_active i32 (-1 on a dropped line), each [rows + cols], rows first.
 *   - status u32[1] is written, not or-ed.
 * lcr_gap_loss_grad: upstream f32[P,2] (d loss / d row term, d column term) -> dS, the layout of S, every element written once by one
 * thread: w_line * ([negative and active] - [positive] * active / count) summed over the element's row line and column line, w_line =
 * upstream / (kept * (hinge + 1)); zero on dropped lines, on the constant entries and at the corner.  Points and transforms get none.
 *
 * lcr_min_dist: stacked queries A f32[na,3] and data D f32[nd,3] in P segments (DEVICE i32[P+1] a_start / d_start; q_max = the host's
 * bound on a segment's query count; a segment that does not fit na / nd is skipped).  dist[q] = sqrt(max(d2, 1e-12f)) of the nearest
 * data point of q's segment, d2 by differences as above; arg i32[na] its segment-local row, the lower row on a tie, -1 (and dist = inf)
 * for an empty segment; mean f32[P] = the mean of dist over the queries with valid[q] != 0 (all of them when valid is NULL), NaN when
 * there is none; count i32[P] = their number.
 * lcr_min_dist_grad: dA[q] = upstream[p] * (a - d*) / dist / count for a valid query whose d2 >= 1e-12f, zero elsewhere.
 *
 * All four are asynchronous, stream-ordered, allocate nothing, use no atomics and give a pair the same bytes alone or in any batch.
 * Domain: 1 <= P <= B <= 65535, n_max, m_max <= 32767, radius >= 0 with (2r)^2 finite in fp32, positive_overlap >= 0; min_dist:
 * 1 <= P <= 65535, na, nd <= (2^31-1)/3.  LCR_EARG outside. */
#define LCR_STATUS_INDEX_RANGE 8u
#define LCR_GAP_LABELS_POINTS 0
#define LCR_GAP_LABELS_OVERLAPS 1
int lcr_gap_loss_ws_bytes(int64_t rows, int64_t cols, size_t* bytes);
int lcr_gap_loss(const float* S, const int64_t* soff, const int64_t* roff, const int64_t* coff, const int32_t* seg_start, int64_t B, int P,
                 int n_max, int m_max, int64_t elems, int64_t rows, int64_t cols, int source, const float* p_pts, const float* q_pts,
                 const float* transforms, double positive_radius, const int64_t* corr, const float* overlaps, const int32_t* corr_start,
                 int64_t C, int64_t c_max, double positive_overlap, const uint8_t* pmask, const uint8_t* qmask, double gamma, float* terms,
                 int32_t* kept, uint8_t* labels, double* line_pos, double* line_hinge, int32_t* line_count, int32_t* line_active,
                 uint32_t* status, void* ws, size_t ws_bytes, void* stream);
int lcr_gap_loss_grad(const float* S, const int64_t* soff, const int64_t* roff, const int64_t* coff, const int32_t* seg_start, int64_t B,
                      int P, int n_max, int m_max, int64_t elems, int64_t rows, int64_t cols, double gamma, const float* upstream,
                      const int32_t* kept, const uint8_t* labels, const double* line_pos, const double* line_hinge,
                      const int32_t* line_count, const int32_t* line_active, float* dS, void* stream);
int lcr_min_dist(const float* A, const int32_t* a_start, int64_t na, const float* D, const int32_t* d_start, int64_t nd,
                 const uint8_t* valid, int P, int64_t q_max, float* dist, int32_t* arg, float* mean, int32_t* count, void* stream);
int lcr_min_dist_grad(const float* A, const int32_t* a_start, int64_t na, const float* D, const int32_t* d_start, int64_t nd,
                      const uint8_t* valid, int P, int64_t q_max, const int32_t* arg, const float* dist, const int32_t* count,
                      const float* upstream, float* dA, void* stream);

/* The Adan optimiser (the reference's experiments/lcrnet/adan.py, arXiv 2208.06677) as ONE pass over a list of fp32 tensors, and the
 * global gradient norm it clips by.  Restated in tests/adan_restatement.py; the Python side is lcrnet_amd.adan.Adan.
 *
 * LcrAdanTensor is a HOST array of T entries: the six DEVICE arrays of one tensor (parameter p, gradient g, exp_avg m, exp_avg_sq n,
 * exp_avg_diff d, pre_grad pg), each numel floats, and `fresh` != 0 for a tensor without a previous gradient (the group's first step, or
 * a parameter that has just gained a gradient).  The table is consumed before the call returns: it is packed into kernel arguments, a
 * few dozen tensors per launch, so nothing is copied to the device, nothing outlives the call and the host never waits.  Pointers need
 * 4-byte alignment only; a tensor whose arrays are all 16-byte aligned moves in 16-byte accesses.  The arrays of a call must not overlap.
 *
 * lcr_adan_grad_norm (g and numel of the entries only): the list is cut into chunks of 4096 elements, tensor after tensor, a tensor's
 *   last chunk being short.  One workgroup per chunk sums (double)g * (double)g in a fixed order into partial[chunk] (ws, fp64); one
 *   workgroup then sums the partials in a fixed order (thread k takes k, k + 256, ... ascending; the 256 sums by a fixed tree) and writes
 *   norm_clip[0] = (float)sqrt(sum) and norm_clip[1] = fminf((float)max_grad_norm / (norm + (float)eps), 1.0f), or 1 when
 *   max_grad_norm == 0 (no clipping).  No atomics: the same gradients give the same bytes on every run, however the launches are cut.
 * lcr_adan_step, per element, fp32 with every operation rounded; the doubles of LcrAdanHyper and 1 - beta_k, 1 -/+ lr * weight_decay
 *   (formed in double) are rounded to fp32 once:
 *     c = clip ? *clip : 1;   g' = c < 1 ? g * c : g            (when c < 1, g' is also stored to g: the reference clips p.grad in place)
 *     diff = fresh ? 0 : g' - pg;   pg = g'
 *     u = g' + beta2 * diff
 *     m = m * beta1 + (1 - beta1) * g';   d = d * beta2 + (1 - beta2) * diff;   n = n * beta3 + ((1 - beta3) * u) * u
 *     den = sqrt(n) / bias3_sqrt + eps
 *     upd = (m / bias1 + (beta2 * d) / bias2) / den
 *     no_prox ?  p = p * (1 - lr * wd) - lr * upd   :   p = (p - lr * upd) / (1 + lr * wd)
 *   bias1 = 1 - beta1^step, bias2 = 1 - beta2^step, bias3_sqrt = sqrt(1 - beta3^step), computed by the caller.  On a fresh tensor pg is
 *   written and never read, and d becomes exactly d * beta2.  clip is a DEVICE float (norm_clip + 1), or NULL for no clipping.
 * Every element is read and written by one thread, so a tensor's result does not depend on the tensors around it.
 * All entries are asynchronous and stream-ordered.  LCR_EARG, launching nothing, for T < 0, numel < 0 or > 2^35, a null pointer with
 * numel > 0, a pointer that is not 4-byte aligned, a negative or NaN max_grad_norm / eps; LCR_ESPACE for a workspace below
 * lcr_adan_ws_bytes.  T == 0 and numel == 0 are legal: no work (the norm of nothing is 0). */
typedef struct {
  float *p, *g, *m, *n, *d, *pg;
  int64_t numel;
  int32_t fresh;
  int32_t pad;
} LcrAdanTensor;
typedef struct {
  double beta1, beta2, beta3, bias1, bias2, bias3_sqrt, lr, weight_decay, eps;
  int32_t no_prox;
  int32_t pad;
} LcrAdanHyper;
int lcr_adan_ws_bytes(const LcrAdanTensor* t, int T, size_t* bytes);
int lcr_adan_grad_norm(const LcrAdanTensor* t, int T, double max_grad_norm, double eps, float* norm_clip, void* ws, size_t ws_bytes,
                       void* stream);
int lcr_adan_step(const LcrAdanTensor* t, int T, const LcrAdanHyper* h, const float* clip, void* stream);

/* TEASER-style robust registration from correspondences (experiments/registration/eval.py:197-218 runs TEASER++ with GNC-TLS rotation and
 * noise_bound 0.01, cbar2 1, gnc_factor 1.4, 100 iterations, cost threshold 1e-12), for S problems in one call (csrc/teaser.hip).  The
 * layout is that of lcr_ransac_correspondences: src / ref f32 [n,3] stacked problem-major, start int32 [S+1], problem s has
 * N = start[s+1] - start[s] rows; the result maps src onto ref.  No TEASER++ binary was available: this text is the contract, the fp64
 * NumPy restatement of tests/teaser_restatement.py the oracle.  All arithmetic is fp64 on the fp32 rows; T is stored as fp32.
 *   1. Consistency graph (mode 0 = kcore).  For i < j: a = |src_j - src_i|, b = |ref_j - ref_i| (sqrt((dx dx + dy dy) + dz dz)); an edge
 *      iff |a - b| <= beta, beta = 2 noise_bound sqrt(cbar2).
 *   2. Selection.  mode 0: the core number of a vertex is the largest k such that it lies in a subgraph of minimum degree k; k_max is
 *      the largest core number and the selected rows are {v : core(v) = k_max} in ascending order (TEASER++'s k-core mode; the exact
 *      maximum clique is not computed).  mode 1 = none: every row is selected, steps 1-2 are skipped and core is written as 0.  K = number
 *      of selected rows.  A problem with k_max < 1 (no edge), K < 3 or N > max_rows is invalid: identity, valid 0, every count 0,
 *      selected_mask 0 (core is still the graph's).
 *   3. Rotation by GNC-TLS over the K (K - 1) / 2 measurements a_m = src_j - src_i, b_m = ref_j - ref_i of all pairs i < j of the selected
 *      rows (not only graph edges).  w = 1, c2 = noise_bound^2, cost_prev = inf; for it = 0 .. max_iterations - 1:
 *        R = rotation_from_H(sum_m w_m a_m b_m^T) (csrc/rigid3.h: V diag(1, 1, det(V U^T)) U^T of the fp64 SVD H = U S V^T);
 *        r_m = |b_m - R a_m|^2;   on it = 0 only: mu = 1 / (2 max_m r_m / c2 - 1), and if not mu > 0: stop and keep R;
 *        th1 = (mu + 1) / mu c2, th2 = mu / (mu + 1) c2, cost = sum_m w_m r_m with the weights that produced R;
 *        w_m = 0 if r_m >= th1, 1 if r_m <= th2, else sqrt(c2 mu (mu + 1) / r_m) - mu;
 *        d = |cost - cost_prev|; mu *= gnc_factor; cost_prev = cost; stop if d < cost_threshold.
 *      rot_inliers = the number of measurements whose final w >= 0.5; iterations = it + 1 at the stop; cost = the last cost (for the stop
 *      at it = 0 on mu: sum_m r_m under that R, with rot_inliers = K (K - 1) / 2).
 *   4. Translation, one axis at a time.  x_v = (ref_v - R src_v)[axis] for the K selected rows, rho = noise_bound sqrt(cbar2).  The 2K
 *      endpoints are listed as x_0 - rho .. x_{K-1} - rho (enter), then x_0 + rho .. x_{K-1} + rho (leave), and sorted by (value, position
 *      in that list).  After each endpoint C is the set of rows that have entered and not left; for every non-empty C
 *      xhat = mean of x over C and cost = sum_C (x - xhat)^2 + rho^2 (K - |C|) (computed from ordered prefix sums of x - x_0 and its square).
 *      The axis estimate is xhat of the smallest cost, the earliest endpoint on ties; t_count[axis] = |C| there.
 *   The bottom row of T is (0, 0, 0, 1) (the reference writes ones into est_transform[3,:3], which no metric reads).
 * max_rows is the caller's bound on the rows of one problem (the entry never reads start on the host); it sizes the workspace and the
 * grids, not the arithmetic: every sum's order depends on its own problem alone, no floating-point atomic is used, so a call returns the
 * same bytes run to run and a problem the same bytes alone or inside any batch.  One kernel form for every size.
 * Outputs: T f32 [S,4,4], valid / n_selected int32 [S], rot_inliers int64 [S], t_count int32 [S,3]; nullable detail: iterations int32 [S],
 * cost f64 [S], selected_mask uint8 [n], core int32 [n].  Rows with a NaN or infinite coordinate give an unspecified transform, never
 * an access outside the tables.
 * 2 (max_iterations + 2) + 5 stream-ordered launches, no host synchronisation: the exit test runs on the device, and a stopped problem's
 * remaining launches exit at once.  Device loops are bounded by max_iterations (GNC) and N rounds (the peel).
 * Domain: 1 <= S <= 65535, 0 <= max_rows <= 4096, 0 <= n <= S max_rows, mode 0 or 1, noise_bound > 0, cbar2 > 0, gnc_factor > 1 (all
 * finite), 1 <= max_iterations <= 1000, 0 <= cost_threshold finite; LCR_EARG with text and no launch outside it, LCR_ESPACE for a
 * workspace below lcr_teaser_ws_bytes (host only: ~ max_rows^2 / 8 + 124 max_rows bytes per problem in mode 0). */
int lcr_teaser_ws_bytes(int S, int64_t n, int max_rows, int mode, size_t* bytes);
int lcr_teaser_registration(const float* src, const float* ref, const int32_t* start, int S, int64_t n, int max_rows, double noise_bound,
                            double cbar2, double gnc_factor, int max_iterations, double cost_threshold, int mode, float* T, int32_t* valid,
                            int32_t* n_selected, int64_t* rot_inliers, int32_t* t_count, int32_t* iterations, double* cost,
                            uint8_t* selected_mask, int32_t* core, void* ws, size_t ws_bytes, void* stream);

/* Scan Context (Kim & Kim, IROS 2018): a polar max-height image per scan, compared under all column shifts; the learning-free loop
 * detector.  Restated in tests/scan_context_restatement.py; parity with the authors' code is not pinned.
 *   Parameters (defaults): R = 20 rings, W = 60 sectors, max_length = 80.0, lidar_height = 2.0.
 *   Descriptor of one cloud.  (x, y, z) is fp32; x and y are promoted to fp64 for the bin decision.
 *     - r = sqrt(x*x + y*y), every operation rounded, no FMA.  theta = atan2(y, x), and theta += 2 pi if theta < 0.
 *     - A point is kept iff r < max_length and z is finite.  Points with a NaN or infinite coordinate therefore drop out.
 *     - ring = min(floor(r / max_length * R), R-1); sector = min(floor(theta / (2 pi) * W), W-1); x = y = 0 goes to bin (0, 0).
 *     - Bin value = the maximum over its points of fl32(z + fl32(lidar_height)); an empty bin holds 0.0f.  A bin whose points are all
 *       below -lidar_height keeps its negative maximum.  desc is f32[R, W].
 *   Derived outputs of the same call.
 *     - ring_key[R] = the fp32 sum of a row, j ascending, divided by fl32(W).
 *     - n_j = sqrtf(sum_i d_ij^2), i ascending in fp32, every operation rounded.  unit_ij = d_ij / n_j where n_j > 0; the whole column is
 *       zero otherwise.  mask is u64: bit j is set iff n_j > 0.
 *   Distance of descriptors a, b at shift s in [0, W).
 *     - V(s) = { j : mask_a[j] and mask_b[(j+s) mod W] }, c(s) = |V(s)|.
 *     - d(s) = 1 - (sum over j in V(s), ascending, of unit_a[:, j] . unit_b[:, (j+s) mod W]) / c(s), or 1 when c(s) = 0.
 *     - dist(a, b) = min_s d(s); shift(a, b) is the smallest minimising s.  This is the paper's exhaustive minimum over all shifts (the
 *       authors' code aligns first with a sector key and searches a few columns around it; that shortcut is not built).
 *     - The column products are fp32 on v_mfma_f32_32x32x2_f32, rings ascending in pairs; the sum over j, the division and the
 *       subtraction are fp32, every operation rounded.
 *   Sign convention: if b is a rotated about +z by phi, then shift ~ phi / (2 pi / W), and Rz(-shift * 2 pi / W) brings b into a's heading.
 *
 * lcr_scan_context: points f32[N,3] stacked cloud-major, lengths HOST int64[B] -> desc f32[B,R,W], ring_key f32[B,R], unit f32[B,R,W],
 *   mask u64[B].  The bin maximum is an integer atomic maximum on an order-preserving map of the fp32 bits, in LDS per workgroup and then
 *   across the workgroups of a cloud: order-free, so a cloud gives the same bytes alone, at any position of a stack, and run to run.
 *   ws: lcr_scan_context_ws_bytes(B, R, W) = 4 B R W bytes rounded up to 256 (the bins being built).
 *   Domain: 1 <= B <= 64, 1 <= R <= 32, 1 <= W <= 64, 0 < max_length finite, lidar_height finite, lengths >= 0, N <= 2^31-1.
 * lcr_scan_context_distance: P pairs (i, j) = pairs[p] (device i32[P,2]) over unit f32[B,R,W] and mask u64[B] -> dist f32[P],
 *   shift i32[P].  A pair with an index outside 0..B-1 reads nothing, gets (NaN, -1) and raises status i32[1] (device) to the largest such
 *   p + 1; status is 0 after a call without one.  P == 0 is legal once B, R, W are in the domain: nothing is launched and status is not
 *   written.  ws: lcr_scan_context_distance_ws_bytes answers 0 (a pair's Gram tile lives in LDS); ws may be NULL.
 *   Domain: 1 <= B <= 2^31-1, 0 <= P <= 2^31-1, R and W as above.
 * lcr_scan_context_topk: the exhaustive causal search, with the semantics of lcr_retrieval_topk.  Query row r is frame q0 + r of
 *   db_unit f32[C,R,W] / db_mask u64[C]; its database is frames [0, q0 + r - exclude).  idx i32[Q,k], dist f32[Q,k], shift i32[Q,k]; a
 *   row is ascending in (dist, index); a row with fewer than k candidates is padded with (-1, +inf, -1).  Q == 0 is legal once the other
 *   arguments are in the domain.  ws: lcr_scan_context_topk_ws_bytes(Q, q0, C, exclude) = 8 Q Cw bytes plus rounding, Cw =
 *   clamp(q0 + Q - 1 - exclude, 0, C) the columns the last row sees: every admissible pair's distance and shift are written once, then
 *   one workgroup per row selects.
 *   Domain: 1 <= C <= 2^31-1, 0 <= Q, 0 <= q0, q0 + Q <= C, exclude >= 0, 1 <= k <= 128, R and W as above.
 * A pair's (dist, shift) has the same bytes in both distance entries, at any position in any call, and run to run: one wavefront computes
 * it by one routine, whatever surrounds it.  No floating-point atomics; every sum has one order.
 * All entries are asynchronous and stream-ordered, allocate nothing and never synchronise with the host; the argument checks and the
 * _ws_bytes helpers are host-only.  LCR_EARG with text and no launch outside a domain (the all-zero call included), LCR_ESPACE for a
 * workspace below the helper's answer. */
int lcr_scan_context_ws_bytes(int B, int R, int W, size_t* bytes);
int lcr_scan_context(const float* points, const int64_t* lengths, int B, int R, int W, double max_length, double lidar_height, float* desc,
                     float* ring_key, float* unit, uint64_t* mask, void* ws, size_t ws_bytes, void* stream);
int lcr_scan_context_distance_ws_bytes(int64_t B, int R, int W, int64_t P, size_t* bytes);
int lcr_scan_context_distance(const float* unit, const uint64_t* mask, int64_t B, int R, int W, const int32_t* pairs, int64_t P, float* dist,
                              int32_t* shift, int32_t* status, void* ws, size_t ws_bytes, void* stream);
int lcr_scan_context_topk_ws_bytes(int64_t Q, int64_t q0, int64_t C, int exclude, size_t* bytes);
int lcr_scan_context_topk(const float* db_unit, const uint64_t* db_mask, int64_t C, int R, int W, int64_t Q, int64_t q0, int k, int exclude,
                          int32_t* idx, float* dist, int32_t* shift, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LCR_HIP_H */
