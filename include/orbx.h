/* orbx.h — C ABI of the MI355X-native ORB front-end (liborbx_hip.so).
 *
 * Drop-in boundary for the two reference classes that own the hot path:
 *   ORB_SLAM3::ORBextractor   /root/reference/include/ORBextractor.h:43-109
 *   ORB_SLAM3::ORBmatcher     /root/reference/include/ORBmatcher.h:36-103  (+ the stereo association that
 *                             Frame runs on the extractor's pyramids, src/Frame.cc:1102-1358, :1530-1587)
 * The reference has no FFI layer of its own: callers use those classes directly.  The C++ facade in
 * include/orb_slam3_amd/ keeps the reference's class names, signatures and return conventions and forwards to
 * the functions below; INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions: plain pointers and sizes only.  Every function returns an int status (0 = ORBX_OK, < 0 =
 * error) unless stated otherwise.  A handle owns one GPU stream pair and all device memory it needs; calls
 * on ONE handle must not overlap in time (the reference never calls one ORBextractor instance
 * concurrently, src/Frame.cc:136-141), calls on DIFFERENT handles may run from different threads.
 * Nothing here ever computes on the CPU: if no GPU / HIP runtime is usable, orbx_create fails.
 */
#ifndef ORBX_H
#define ORBX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBX_OK 0
#define ORBX_E_EMPTY (-1)      /* empty image: ORBextractor::operator() returns -1, src/ORBextractor.cc:1561-1562 */
#define ORBX_E_ARG (-2)        /* bad argument / image too small for the 35-px FAST cell grid */
#define ORBX_E_DEVICE (-3)     /* HIP error (no device, allocation or launch failure) */
#define ORBX_E_CAPACITY (-4)   /* caller buffer too small (n_out still reports the required size) */
#define ORBX_E_INTERNAL (-5)   /* device-side capacity check tripped */

/* cv::KeyPoint as the reference fills it (src/ORBextractor.cc:1184-1198, :587): 28 bytes */
typedef struct OrbxKeyPoint {
    float x, y;        /* level-0 pixel coordinates (level coords * mvScaleFactor[octave]) */
    float size;        /* int(31 * scale) */
    float angle;       /* degrees [0,360], cv::fastAtan2 of the intensity-centroid moments */
    float response;    /* FAST corner score (OpenCV cornerScore), NOT a Harris score */
    int32_t octave;
    int32_t class_id;  /* always -1 */
} OrbxKeyPoint;

typedef struct orbx_extractor orbx_extractor;

/* number of usable GPUs (0 if none) */
int orbx_device_count(void);
/* How the host threads of this process wait for GPU `device_id` inside the synchronous calls (orbx_extract, orbx_fetch, orbx_sync, the orbm_* searches):
 * 0 = the HIP runtime's default (the waiting thread spins: lowest latency - one pair per call is 0.127 ms - and one host core per waiting thread),
 * 1 = blocking (the thread sleeps on the completion interrupt: a wake-up of ~10 - 20 us per wait and no core: what a host that runs one process per GPU on
 * fewer cores than 2 x GPUs wants - bench.py --gpus N uses it for N > 1), 2 = spin, 3 = yield.  Process-wide per device (hipSetDeviceFlags). */
int orbx_set_host_wait(int device_id, int mode);

/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)  include/ORBextractor.h:49-50,
 * src/ORBextractor.cc:468-571.  device_id selects the GPU (one process per GPU in multi-GPU runs).
 * Limits, all reported loudly: images of at most 4127 x 4127 pixels and at least the 35-px FAST cell grid on the smallest level (ORBX_E_ARG from the
 * extraction); fewer than 65 535 keypoints per image over all levels (16-bit node indices; the reference's settings files ask for 500 - 2 000 and
 * Tracking builds its monocular initialisation extractor with five times that, src/Tracking.cc:634-635, :1331-1332: up to 10 000).
 * The quadtree of a level (src/ORBextractor.cc:711-1057) works in LDS when its node lists fit - 81 bytes per node beside 16 - 55 KB of bucket
 * counters and coordinate tables: with the 160 KB of gfx950 that is every level of up to ~1 400 - 1 800 keypoints, i.e. every level of every stereo,
 * RGB-D and post-initialisation monocular setting - and in a global node pool otherwise (level 0 of 10 000 features at 1241 x 376 holds 2 172):
 * the same algorithm and the same result, without a bound of its own. */
int orbx_create(orbx_extractor** out, int nfeatures, float scale_factor, int nlevels,
                int ini_th_fast, int min_th_fast, int device_id);
void orbx_destroy(orbx_extractor* h);

/* Which 8-bit 7x7 sigma=2 Gaussian the linked OpenCV would apply (src/ORBextractor.cc:1632):
 * 0 = OpenCV >= 3.4/4.x fixed-point path, taps [18,34,48,56,48,34,18]/256 (default)
 * 1 = OpenCV 3.2 integer separable filter, taps [18,34,49,55,49,34,18]/256 */
int orbx_set_gaussian_taps(orbx_extractor* h, int variant);

/* Pre-allocate for images of width x height and batches up to max_batch (otherwise done lazily). */
int orbx_reserve(orbx_extractor* h, int width, int height, int max_batch);

/* Getters of include/ORBextractor.h:61-81 (by value in the reference). */
int orbx_get_levels(const orbx_extractor* h);
float orbx_get_scale_factor(const orbx_extractor* h);
int orbx_get_level_tables(const orbx_extractor* h, float* scale, float* inv_scale, float* sigma2,
                          float* inv_sigma2, int* features_per_level, int* umax16);
/* Upper bound of keypoints per image (nfeatures + 3 per level, src/ORBextractor.cc:912,1006): size output buffers with it. */
int orbx_max_keypoints(const orbx_extractor* h);

/* ORBextractor::operator()(image, mask, keypoints, descriptors, vLappingArea)  include/ORBextractor.h:57-59,
 * src/ORBextractor.cc:1557-1682.  image: 8-bit grey, host memory.  kps: cap records, desc: cap x 32 bytes (row i <->
 * keypoint i).  *n_out = number of keypoints, *mono_index_out = the reference's return value (monoIndex).
 * Blocking (the reference call is synchronous). */
int orbx_extract(orbx_extractor* h, const uint8_t* image, int width, int height, int stride,
                 int lap0, int lap1, OrbxKeyPoint* kps, uint8_t* desc, int cap,
                 int* n_out, int* mono_index_out);

/* Batched form: B independent images of identical size, image b at images + b*image_stride.
 * images_on_device != 0: `images` is device memory of this handle's GPU (see orbx_device_alloc).
 * Asynchronous: enqueues on the handle's stream; results stay resident on the device for orbx_fetch and
 * for the orbm_* matchers.  */
int orbx_extract_batch(orbx_extractor* h, int B, const uint8_t* images, int width, int height, int stride,
                       size_t image_stride, int images_on_device, int lap0, int lap1);
/* Copy the results of the last batch to the host (blocking).  kps: [B][cap], desc: [B][cap][32], n_out/mono_out: [B].
 * Waits for the extraction and for its own copies, not for what was queued on the handle behind the extraction: after a batch of more than 32
 * images the download runs beside a matcher enqueued before this call (orbm_stereo_match, ...), whose own fetch waits for it. */
int orbx_fetch(orbx_extractor* h, OrbxKeyPoint* kps, uint8_t* desc, int cap, int* n_out, int* mono_out);
int orbx_sync(orbx_extractor* h);

/* mvImagePyramid[level] of image `image_index` of the last batch (public member include/ORBextractor.h:83; the
 * un-bordered level — the 19-px reflect border is never read by the hot path).  blurred != 0 returns the
 * GaussianBlur'ed level used for the descriptors.  dst may be NULL to query the size. */
int orbx_pyramid_level(orbx_extractor* h, int image_index, int level, int blurred, uint8_t* dst,
                       int dst_stride, int* width, int* height);
/* all levels of one image with a single device-to-host copy: dst[l] receives level l (width x height of orbx_pyramid_level) with row pitch dst_stride[l] */
int orbx_pyramid_fetch(orbx_extractor* h, int image_index, int blurred, uint8_t* const* dst, const int* dst_stride);
/* Bordered pyramid export (ORB-SLAM3's mvImagePyramid, src/ORBextractor.cc:1687-1738).  edge > 0: every later extraction also writes each
   level of each image as a (w + 2*edge) x (h + 2*edge) frame, level at (edge, edge), BORDER_REFLECT_101 around it, into page-locked memory
   of the handle, overlapped with the rest of the extraction.  What extraction k exported stays valid until extraction k + depth is enqueued
   (or the geometry changes, or a larger batch than any before grows the slots).  edge = 0 turns the export off and frees the slots.
   edge <= 256, depth 1..8; the border repeats its reflection where edge exceeds a level's size.  orbx_fetch does not wait for the export,
   orbx_sync does.  Under orbx_set_graph_replay the export runs behind the replayed graph instead of beside it. */
int orbx_set_pyramid_export(orbx_extractor* h, int edge, int depth);
/* Waits for image b of the last extraction; level l's frame starts at base + offset[l], pitch step[l], level size width[l] x height[l]
   (arrays of orbx_get_levels(h) entries; every output may be NULL).  Refused when the last extraction exported nothing. */
int orbx_pyramid_exported(orbx_extractor* h, int b, const uint8_t** base, size_t* offset, int* step, int* width, int* height);

/* device memory helpers so a caller can keep inputs resident (bench, multi-camera rigs) */
int orbx_device_alloc(orbx_extractor* h, size_t bytes, void** dptr);
int orbx_device_free(orbx_extractor* h, void* dptr);
int orbx_device_upload(orbx_extractor* h, void* dptr, const void* host, size_t bytes);
/* the same on the handle's copy stream, without waiting: the next orbx_extract_batch(..., on_device = 1) of this handle waits for it on the
 * device, and the copy itself waits until the previous extraction has read its input (upload batch i + 1 while batch i is processed;
 * `host` should be page-locked, orbx_host_alloc) */
int orbx_device_upload_async(orbx_extractor* h, void* dptr, const void* host, size_t bytes);

/* Frame::UndistortKeyPoints (src/Frame.cc:1003-1034) on the device: with K = (fx, fy, cx, cy) and dist = mDistCoef (k1, k2, p1, p2[, k3]; ndist 4 or 5)
 * every extraction also produces mvKeysUn - cv::undistortPoints(keys, K, dist, R = empty, P = K) in OpenCV's double arithmetic (restated;
 * opencv_variant 0 = OpenCV >= 3.4.2, 1 = 3.2) - for orbx_fetch_undistorted and for the device-resident consumers (orbm_stereo_from_depth,
 * orbm_search_local_points_batch).  dist == NULL or dist[0] == 0: mvKeysUn = mvKeys, as the reference decides (:1005-1009).
 * orbx_undistorted_bounds = Frame::ComputeImageBounds (:1043-1075): out = mnMinX, mnMaxX, mnMinY, mnMaxY. */
int orbx_set_undistort(orbx_extractor* h, const float K[4], const float* dist, int ndist, int opencv_variant);
int orbx_fetch_undistorted(orbx_extractor* h, OrbxKeyPoint* kps_un, int cap);       /* [B][cap], blocking */
int orbx_undistorted_bounds(const orbx_extractor* h, int width, int height, float out[4]);

/* Zero-copy input: the address and layout of pyramid level 0 inside the handle, for B images of width x height (reserves like orbx_reserve).
 * A producer that can write there - a camera DMA, a decoder, orbx_input_upload below - hands its frames over without the import pass
 * (one read and one write of every pixel): call orbx_extract_batch(h, B, *dptr, width, height, *stride, *image_stride, 1, ...) with exactly
 * these values and the extraction reads level 0 in place.  Image b starts at dptr + b * image_stride, rows are `stride` bytes apart; bytes
 * beyond `width` in a row are padding: write ONLY bytes [0, width) of a row.  The padding was zeroed when the buffer was laid out and the
 * kernels load it as part of whole dwords; no output depends on its value (tests/test_emu_parity.py: test_zero_copy_input_garbage_padding_* fill it with garbage), but a
 * producer that copies full-pitch rows makes every run read bytes it does not control.  The buffer stays valid until the handle is reconfigured for another size or a larger batch; level 0
 * is never written by the extraction, so a resident batch can be extracted repeatedly. */
int orbx_input_buffer(orbx_extractor* h, int width, int height, int B, void** dptr, int* stride, size_t* image_stride);
/* B host images (stride / image_stride as in orbx_extract_batch) into that buffer; blocking */
int orbx_input_upload(orbx_extractor* h, int B, const uint8_t* images, int width, int height, int stride, size_t image_stride);

/* device addresses of the results of the last batch: keypoints [B][cap] (28-byte records), descriptors [B][cap][32] (rows beyond n[b] are
 * zero), n [B], monoIndex [B]; valid until the next extraction / reconfiguration of the handle (synchronise with orbx_sync first).  For
 * consumers that stay on the device, e.g. an RCCL all-gather of the descriptor blocks (orb_slam3_detailed_comments_amd/multi.py). */
int orbx_device_outputs(orbx_extractor* h, void** kps, void** desc, void** n, void** mono, int* cap, int* B);
/* A SNAPSHOT of the descriptor blocks and counts of the last batch in device memory the CALLER owns (desc_dst: B * cap * 32 bytes, n_dst: B ints,
 * either may be NULL): device-to-device copies on the handle's stream behind the extraction, complete when the call returns.  The handle's own
 * buffers are rewritten by its next extraction, so a consumer that overlaps that extraction (an asynchronous collective) works on a snapshot. */
int orbx_device_snapshot(orbx_extractor* h, void* desc_dst, void* n_dst);
/* ---- the exchange step of the multi-GPU mode (BASELINE.json configs[4]) ----
 * Streams are independent: one process (or thread) per GPU, each with its own extractor / matcher handles created with that GPU's device_id,
 * and no collective on the hot path.  The ONE exchange a host may want - every rank's descriptor blocks on every rank, in front of a global
 * matcher - is an all-gather over RCCL / xGMI, offered here so that a C++ host needs neither Python nor torch.distributed:
 *   rank 0:      orbx_comm_unique_id(id)  ->  id reaches the other ranks by whatever the host has (MPI, a socket, a file, torch.distributed)
 *   every rank:  orbx_comm_create(&c, world, rank, id, device_id)         (collective: ncclCommInitRank; or orbx_comm_adopt for an ncclComm_t it owns)
 *   per batch:   orbx_extract_batch(h, ...); orbx_allgather_descriptors(h, c, &desc_all, &n_all, &B, &cap);  ...next extraction...;  orbx_comm_wait(c)
 * orbx_allgather_descriptors snapshots the descriptor block [B][cap][32] (rows beyond n[b] zero) and the counts [B] of h's last batch behind the
 * extraction, then gathers both over the communicator's own stream: ASYNCHRONOUS - the handle may extract its next batch at once.  desc_all
 * [world][B][cap][32] and n_all [world][B] are device memory of the communicator, valid after orbx_comm_wait and until the next call; every
 * rank must gather blocks of the same shape (same B, same extractor geometry).  orbx_comm_fetch waits and copies them to the host.
 * A call that finds the communicator's previous exchange still in flight does not wait for it on the host: its snapshot is ordered behind that exchange
 * on the device (several handles may share one communicator).  The gathered blocks are double-buffered: what a call returned is written again by the
 * SECOND call after it, not by the next one, so a consumer of exchange k (on a stream of its own, after orbx_comm_wait) may run beside exchange k + 1;
 * n_all sits behind desc_all at world * B * cap * 32 bytes - take both pointers from the call, they move when B changes.  After a failed call
 * orbx_comm_fetch refuses (nothing was gathered).
 * librccl is loaded (dlopen) by the first orbx_comm_* call; hosts that never call them never load it. */
typedef struct orbx_comm orbx_comm;
#define ORBX_COMM_ID_BYTES 128            /* sizeof(ncclUniqueId) */
int orbx_comm_unique_id(uint8_t id[ORBX_COMM_ID_BYTES]);
int orbx_comm_create(orbx_comm** c, int world, int rank, const uint8_t id[ORBX_COMM_ID_BYTES], int device_id);
int orbx_comm_adopt(orbx_comm** c, void* nccl_comm /* ncclComm_t of the caller, not destroyed by orbx_comm_destroy */, int world, int rank, int device_id);
void orbx_comm_destroy(orbx_comm* c);
int orbx_comm_world(const orbx_comm* c);
int orbx_comm_rank(const orbx_comm* c);
int orbx_allgather_descriptors(orbx_extractor* h, orbx_comm* c, void** desc_all, void** n_all, int* B, int* cap);   /* out pointers may be NULL */
int orbx_comm_wait(orbx_comm* c);
int orbx_comm_fetch(orbx_comm* c, uint8_t* desc_all_host, int* n_all_host);                                           /* either may be NULL */

/* GPU index the handle was created on; ORBX_DEVICE_HOST when the library's "device" memory is plain host memory (only the CPU emulator build of
 * the kernel sources that the tests use - the product library never returns it) */
#define ORBX_DEVICE_HOST (-1)
int orbx_device_id(const orbx_extractor* h);
/* page-locked host memory for output buffers: with cap == orbx_max_keypoints() orbx_fetch / orbm_stereo_fetch copy straight
 * into the caller's arrays (no staging, no repacking) and pinned memory makes that copy run at PCIe speed */
int orbx_host_alloc(orbx_extractor* h, size_t bytes, void** hptr);
int orbx_host_free(orbx_extractor* h, void* hptr);

/* How ComputePyramid (src/ORBextractor.cc:1687-1738) is launched: 0 (default) = by batch size - all levels in one launch for small
 * batches, where a chain of one launch per level is pure launch latency, one streaming launch per level for large ones; 1 / 2 force
 * either form (tests compare them).  The levels are bit-identical in every mode. */
int orbx_set_pyramid_mode(orbx_extractor* h, int mode);

/* Small batches (up to 32 images per call; one stereo pair per call is Tracking's rhythm) are launch-latency bound and run a launch form of
 * their own: the blur strips and the FAST cells in ONE launch on one stream (large batches: two launches on two streams, i.e. a fork and a
 * join of ~6 us each).  on = 1 (default) / 0 = the large-batch form at every batch size (tests compare them: the outputs are bit-identical).
 * The profiling modes (orbx_profile_enable) time stages and always run the large-batch form. */
int orbx_set_small_batch_forms(orbx_extractor* h, int on);

/* Replay the extraction pipeline as one hipGraph (captured on first use, re-captured when the batch size, geometry, input
 * pointer or lapping area change).  Pays off at small batches, where the ~17 kernel launches are latency-bound. */
int orbx_set_graph_replay(orbx_extractor* h, int on);

/* Per-stage GPU time of the last batch, HIP events on the launching streams.  on = 1: normal two-stream schedule (the blur
 * overlaps FAST + quadtree, so their times overlap too); on = 2: serial schedule, every kernel alone on one stream. */
#define ORBX_NSTAGES 8
int orbx_profile_enable(orbx_extractor* h, int on);
int orbx_profile_get(orbx_extractor* h, float ms[ORBX_NSTAGES]);
const char* orbx_stage_name(int i);

/* Stage probes for parity tests (level-ordered intermediate results of image `image_index`). */
int orbx_debug_candidates(orbx_extractor* h, int image_index, int level, int* xys, int cap);       /* returns count; (x,y,score) rel. to the 16-px border, reference order */
int orbx_debug_level_keys(orbx_extractor* h, int image_index, int level, int* xys, int cap);       /* quadtree output in list order */
/* test switches of the stereo row search (orbm_stereo_match): bit 0 visits the candidates of a row band in the opposite order (the result
 * must not change), bit 2 makes every lane walk all candidates from the last to the first (every tie then meets inside one lane; the
 * result must not change either), bit 1 restores the distance-only tie rule of an earlier revision (the tie tests must then fail);
 * bit 3: the 2-NN of orbm_knn2 / orbm_stereo_fisheye on the vector units (one wave per query) instead of the matrix cores (the result must
 * not change); bit 4: orbm_project_points and orbm_search_by_projection_lastframe_batch evaluate `Tcw * p` as q.toRotationMatrix() * p + t
 * (an earlier revision's form) instead of Sophus' quaternion action (tests/test_sophus_action.py: the reference must then catch it) */
int orbx_debug_stereo_flags(orbx_extractor* h, int flags);
int orbx_debug_quadtree_profile(orbx_extractor* h, long long out[16]);   /* phase timestamps of one quadtree workgroup (profiling mode 2) */
/* test hook: the largest quadtree (nodes per level) that is given the LDS form; levels above it keep their node lists in the global node pool
 * (the form the 5 x nFeatures extractor of the monocular initialisation takes for its first levels).  0 = every level in the pool; the default and
 * the largest value is 4 000.  Bit-identical outputs. */
int orbx_debug_quadtree_lds_nodes(orbx_extractor* h, int max_nodes);
int orbx_debug_quadtree_pool_levels(orbx_extractor* h);                   /* number of levels (0 .. n-1) the last extraction ran in the pool form */
/* test hook: the quadtree moves a level's keys into sorted order only when it divides a node at or below the depth of its up-front counting sort.
 * on != 0: every tree sorts right after the gather, as before that change (A/B runs).  Bit-identical outputs. */
int orbx_debug_quadtree_eager(orbx_extractor* h, int on);
/* per_level[0 .. levels-1] of image image_index of the last extraction: why the level's tree sorted its keys - 0 never, 1 first needed in a full pass,
 * 2 first needed in a final round, 3 at once (the switch above, or a level outside the lazy form's limits) */
int orbx_debug_quadtree_sorted(orbx_extractor* h, int image_index, int* per_level);
/* test hook: the byte / packed-16-bit instruction wrappers of the kernels (csrc/orbx_simd.h) applied to n operand triples (n a multiple of 256);
 * out = 22 x n results in the order mul24, mul24 (forced), v_perm_b32, v_alignbyte_b32, v_dot4_u32_u8, v_dot2_u32_u16, packed max3, packed min3,
 * packed sub, packed xor(a, c), wave inclusive scan / wave sum of a & 0xFFFF, wave minimum of b (per 64 consecutive elements), v_sad_u8, v_mul_u32_u24,
 * the 64-bit wave scan (two words), the 64-bit workgroup scan (two words), the wave OR, v_mul_hi_u32_u24, v_add3_u32 */
int orbx_debug_simd_selftest(orbx_extractor* h, const uint32_t* a, const uint32_t* b, const uint32_t* c, int n, uint32_t* out);
/* test hook: the device build of the bit-exact function models (csrc/glibc_*_model.h, cv::fastAtan2 in csrc/k_describe.hip) evaluated on n inputs,
 * 1 <= n <= 1 << 26, one thread per element (tests/test_model_sweep.py walks whole float domains with it).  With a == NULL input i is the float whose
 * bit pattern is start_bits + i (ops 0 .. 4 only); otherwise input i is a[i], with b[i] as the second operand of ops 5 .. 7.  Host buffers.
 *  op 0 cosf, 1 sinf, 2 logf, 3 tanf, 4 atanf, 5 atan2f(a, b), 6 fastAtan2(a, b) in degrees: out = n results;
 *  op 7 the steering of a keypoint with the patch moments m01 = a, m10 = b, by the function the descriptor kernel calls:
 *       out = 3 n floats, out[i] = angle, out[n + i] = cosf(angle * pi / 180), out[2 n + i] = sinf(..). */
int orbx_debug_model_eval(orbx_extractor* h, int op, uint32_t start_bits, const float* a, const float* b, int n, float* out);
/* test hook: the workgroup primitives of the quadtree kernel (csrc/k_quadtree.hip) run by ONE workgroup of `threads` threads (256 or 1024, the two
 * sizes a tree runs on) on the caller's data, with their arrays laid out as a tree lays them out.  Host buffers.
 *  ORBX_QT_SELFTEST_SORT: in = n 64-bit keys, out = the n keys after the kernel's model of libstdc++'s std::sort with the comparator
 *    (a >> 16) < (b >> 16) - the final rounds' order of (count << 32 | x0 << 16 | index).  spill = 0: every array in LDS, n <= 4095; spill = 1: the
 *    node-pool form (arrays in device memory, 20-bit range positions), n <= 65535.  start, total, mx, my are not used.
 *  ORBX_QT_SELFTEST_PARTITION4: in = `total` 32-bit keys (x | y << 12 | ..), out = `total` keys + 4 counts.  The span [start, start + n) of `in` is
 *    partitioned stably into the same span of `out`, children n1|n2|n3|n4 with left = x < mx, top = y < my; out[total .. total + 4) = the four counts.
 *    `out` comes in filled: its first `total` keys are uploaded first and everything outside the span has to come back unchanged.  start >= 1.
 *  ORBX_QT_SELFTEST_SCAN: in = n = `threads` 64-bit values, out = the exclusive prefix sum per thread + the total (threads + 1 values). */
#define ORBX_QT_SELFTEST_SORT 0
#define ORBX_QT_SELFTEST_PARTITION4 1
#define ORBX_QT_SELFTEST_SCAN 2
int orbx_debug_quadtree_selftest(orbx_extractor* h, int op, int spill, int threads, const void* in, int n, int start, int total, int mx, int my, void* out);
/* what the library holds at this moment, process-wide: out = { device allocations, page-locked host allocations, streams, events }.  The lifetime
 * tests create, use and destroy every kind of handle (extractor, key frames, map points, vocabulary, communicator, caller buffers) and expect the
 * four counts back where they started (tests/test_lifetime.py). */
int orbx_debug_live_resources(long long out[4]);

/* ---------------------------------------------------------------------------------------------------------- */
/* ORBmatcher::DescriptorDistance (include/ORBmatcher.h:44, src/ORBmatcher.cc:2383-2403), all pairs:
 * out[i*nb + j] = Hamming(a[i], b[j]).  Host buffers; runs on the handle's GPU. */
int orbm_hamming_matrix(orbx_extractor* h, const uint8_t* a, int na, const uint8_t* b, int nb, int* out);

/* Frame::ComputeStereoMatches (src/Frame.cc:1102-1358) for B rectified pairs: pair p uses image
 * left_first+p of `left`'s last batch and image right_first+p of `right`'s last batch (left == right is allowed:
 * one handle that extracted [L0..LB-1, R0..RB-1]).  bf = mbf, b = mb (include/Frame.h:209-212).  Asynchronous. */
int orbm_stereo_match(orbx_extractor* left, int left_first, orbx_extractor* right, int right_first,
                      int B, float bf, float b);
/* uRight/depth: [B][cap] (mvuRight / mvDepth, -1 = none), n_matches: [B].  Blocking. */
int orbm_stereo_fetch(orbx_extractor* left, int B, float* uRight, float* depth, int cap, int* n_matches);

/* Matching part of Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1553-1562): brute-force Hamming 2-NN of
 * left[monoLeft:] against right[monoRight:] + Lowe ratio (0.7).  Outputs [B][cap], indexed by query row
 * relative to monoLeft; idx relative to monoRight (DMatch.queryIdx/trainIdx).  Blocking fetch. */
int orbm_knn2(orbx_extractor* left, int left_first, orbx_extractor* right, int right_first, int B);
int orbm_knn2_fetch(orbx_extractor* left, int B, int* idx0, int* dist0, int* idx1, int* dist1,
                    uint8_t* ratio_ok, int cap);

/* Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1530-1587) for B fisheye pairs whose two images were extracted with the cameras' lapping
 * areas: brute-force 2-NN + ratio test on the lapping keypoints, then KannalaBrandt8::TriangulateMatches (parallax, DLT triangulation,
 * positive depth in both cameras, reprojection chi-square; src/CameraModels/KannalaBrandt8.cpp:439-523) on every survivor; accepted when
 * the depth is > 1e-4.  Asynchronous; orbm_stereo_fisheye_fetch returns, per pair, mvLeftToRightMatch [cap], mvRightToLeftMatch [cap],
 * mvDepth [cap] (-1 = none), mvStereo3Dpoints [cap][3] and the number of matches.  The null vector of the triangulation matrix is computed
 * in fp64 instead of Eigen's fp32 JacobiSVD: depths agree with the reference to ~1e-6 relative, not bit for bit. */
typedef struct OrbmKB8Stereo {
    float cam1[8], cam2[8];               /* KannalaBrandt8::mvParameters (fx, fy, cx, cy, k0..k3) of mpCamera and mpCamera2 */
    float R12[9], t12[3];                 /* Frame::mRlr (row-major), mtlr */
} OrbmKB8Stereo;
int orbm_stereo_fisheye(orbx_extractor* left, int left_first, orbx_extractor* right, int right_first, int B, const OrbmKB8Stereo* cams);
int orbm_stereo_fisheye_fetch(orbx_extractor* left, int B, int* l2r, int* r2l, float* depth, float* p3d, int* n_matches, int cap);

/* ---------------------------------------------------------------------------------------------------------- */
/* Guided searches.  The reference methods take Frame / KeyFrame / MapPoint objects (pointer graphs with mutexes);
 * across the C ABI they are passed as read-only structure-of-arrays VIEWS of exactly the fields the method reads.
 * The facade (include/orb_slam3_amd/ORBmatcher.h) fills the views from the real classes and applies the results.
 * Geometry that the reference computes with Eigen/Sophus before matching (Tcw * x3Dw, GeometricCamera::project,
 * the fundamental matrix) stays on the caller's side and enters here as numbers, so its float op order is the
 * reference's own.  The functions below are the Frame::Nleft == -1 paths; the two-camera (fisheye rig) branches of the two
 * SearchByProjection overloads are the *_fisheye entry points further down. */
typedef struct OrbmFrameView {            /* fields of ORB_SLAM3::Frame, include/Frame.h */
    int N;                                /* number of keypoints */
    const OrbxKeyPoint* keys_un;          /* mvKeysUn (:232) */
    const uint8_t* desc;                  /* mDescriptors, N x 32 (:244) */
    const float* u_right;                 /* mvuRight, negative = monocular point (:234); NULL = all monocular */
    const uint8_t* occupied;              /* mvpMapPoints[i] != NULL && mvpMapPoints[i]->Observations() > 0 */
    float min_x, min_y, max_x, max_y;     /* mnMinX .. mnMaxY (:287-290) */
    float grid_w_inv, grid_h_inv;         /* mfGridElementWidthInv / HeightInv (:250-251) */
    float mbf;                            /* (:209) */
    int nlevels; const float* scale_factors;   /* mvScaleFactors (:281) */
} OrbmFrameView;

typedef struct OrbmMapPointView {         /* tracking fields of ORB_SLAM3::MapPoint, include/MapPoint.h:171-179 */
    int M;
    const uint8_t* in_view;               /* mbTrackInView */
    const float* proj_x; const float* proj_y; const float* proj_xr;   /* mTrackProjX / Y / XR */
    const int* scale_level;               /* mnTrackScaleLevel */
    const float* view_cos;                /* mTrackViewCos */
    const float* track_depth;             /* mTrackDepth */
    const uint8_t* is_bad;                /* isBad() */
    const uint8_t* has_obs;               /* Observations() > 0 */
    const uint8_t* desc;                  /* GetDescriptor(), M x 32 */
} OrbmMapPointView;

/* Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel) (src/Frame.cc:859-951): indices in the reference's order.
 * Returns the count (>= 0) or a negative status. */
int orbm_get_features_in_area(orbx_extractor* h, const OrbmFrameView* F, float x, float y, float r,
                              int min_level, int max_level, int* indices, int cap);

/* ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints)
 * (src/ORBmatcher.cc:45-239).  assigned[i] = index of the map point written to F.mvpMapPoints[i], or -1 if the call
 * leaves that entry untouched.  *nmatches = the reference's return value. */
int orbm_search_by_projection_mappoints(orbx_extractor* h, const OrbmFrameView* F, const OrbmMapPointView* P,
                                        float th, int far_points, float th_far_points, float nnratio,
                                        int* assigned, int* nmatches);

typedef struct OrbmLastFrameView {        /* what SearchByProjection(CurrentFrame, LastFrame, ...) reads of LastFrame */
    int N;
    const uint8_t* valid;                 /* mvpMapPoints[i] != NULL && !mvbOutlier[i] && invzc >= 0 && projection inside bounds */
    const float* proj_u; const float* proj_v;   /* CurrentFrame.mpCamera->project(Tcw * pMP->GetWorldPos()) */
    const float* inv_z;                   /* 1 / x3Dc(2) */
    const int* octave;                    /* LastFrame.mvKeys[i].octave */
    const float* angle;                   /* LastFrame.mvKeysUn[i].angle */
    const uint8_t* has_obs;               /* pMP->Observations() > 0 */
    const uint8_t* desc;                  /* pMP->GetDescriptor(), N x 32 */
} OrbmLastFrameView;

/* C1 on the device: Frame::isInFrustum (src/Frame.cc:667-773, one camera) + Pinhole / KannalaBrandt8::project + MapPoint::PredictScale
 * (src/MapPoint.cc:688-731) for M map points at once, in the reference's fp32 operation order (mRcw * P + mtcw as a matrix product, as the
 * reference writes it; Eigen >= 3.3 - which the vendored Sophus requires - sums the three terms of a product coefficient, a dot() or a
 * norm() as a0 + (a1 + a2); no fused multiply-adds).  The outputs are the fields the reference stores in the
 * MapPoint: mbTrackInView, mTrackProjX / Y / XR, mTrackDepth, mTrackViewCos, mnTrackScaleLevel (`out` itself is required; any array pointer in
 * it may be NULL).  MapPoint::PredictScale's log is glibc's logf (the reference's std::log(float)), reproduced bit for bit on the device. */
typedef struct OrbmFrustumView {
    float Rcw[9], tcw[3], Ow[3];          /* Frame::mRcw (row-major) = mTcw.rotationMatrix(), mtcw, mOw = mTcw.inverse().translation() (src/Frame.cc:594-598) */
    float qcw[4];                         /* mTcw.unit_quaternion().coeffs() (x, y, z, w): read by orbm_search_by_projection_lastframe_batch only, which
                                           * evaluates `Tcw * x3Dw` (src/ORBmatcher.cc:1987) as Sophus does - on the quaternion, not on mRcw */
    int camera_type;                      /* GeometricCamera::GetType(): 0 pinhole (cam = fx, fy, cx, cy), 1 Kannala-Brandt (8 parameters) */
    float cam[8];
    float min_x, max_x, min_y, max_y;     /* mnMinX .. mnMaxY */
    float mbf, log_scale_factor;          /* mbf, mfLogScaleFactor */
    int nlevels; const float* scale_factors;
} OrbmFrustumView;
typedef struct OrbmWorldPointView {       /* map points by position */
    int M;
    const float* pos;                     /* GetWorldPos(), M x 3 */
    const float* normal;                  /* GetNormal(), M x 3 */
    const float* min_distance;            /* mfMinDistance (GetMinDistanceInvariance() / 0.8) */
    const float* max_distance;            /* mfMaxDistance (GetMaxDistanceInvariance() / 1.2) */
    const uint8_t* is_bad;                /* isBad() (NULL = none) */
    const uint8_t* has_obs;               /* Observations() > 0 (NULL = all) */
    const uint8_t* desc;                  /* GetDescriptor(), M x 32 (searches only) */
} OrbmWorldPointView;
typedef struct OrbmTrackOut { uint8_t* in_view; float *proj_x, *proj_y, *proj_xr, *depth, *view_cos; int* scale_level; } OrbmTrackOut;
int orbm_is_in_frustum(orbx_extractor* h, const OrbmFrustumView* frame, const OrbmWorldPointView* points, float viewing_cos_limit, const OrbmTrackOut* out);
/* isInFrustum for every point, then ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) (src/ORBmatcher.cc:45-167)
 * on the points in view, as Tracking::SearchLocalPoints does (src/Tracking.cc:4009-4067): the window queries are produced and consumed on
 * the device.  assigned[i] = index of the map point given to keypoint i, or -1; out (may be NULL) receives the tracking fields. */
int orbm_search_local_points(orbx_extractor* h, const OrbmFrameView* F, const OrbmFrustumView* frame, const OrbmWorldPointView* points,
                             float viewing_cos_limit, float th, int far_points, float th_far, float nnratio, const OrbmTrackOut* out,
                             int* assigned, int* nmatches);

/* The same with the map points resident on the device: Tracking::SearchLocalPoints visits the local map (2 000 - 6 000 points,
 * Tracking::UpdateLocalPoints, src/Tracking.cc:4070-4110) every frame, and a map point's position, normal, distance limits and descriptor
 * change only when LocalMapping / LoopClosing touch it.  orbm_points_create uploads those fields of a point set once (is_bad / has_obs of the
 * view are ignored: they are call-time state); orbm_search_local_points_resident then moves the frame, the two flag arrays (NULL: no point bad /
 * every point observed) and the results only.  Same results as orbm_search_local_points. */
typedef struct orbm_points orbm_points;
int orbm_points_create(orbx_extractor* h, const OrbmWorldPointView* points, orbm_points** out);
void orbm_points_destroy(orbm_points* p);
int orbm_search_local_points_resident(orbx_extractor* h, const OrbmFrameView* F, const OrbmFrustumView* frame, const orbm_points* points,
                                      const uint8_t* is_bad, const uint8_t* has_obs, float viewing_cos_limit, float th, int far_points, float th_far,
                                      float nnratio, const OrbmTrackOut* out, int* assigned, int* nmatches);

/* Frame::ComputeStereoFromRGBD (src/Frame.cc:1361-1391) for frames [first, first + B) of the handle's last extraction: mvDepth[i] = the depth
 * image (CV_32F, already scaled by Tracking::mDepthMapFactor, src/Tracking.cc:1617-1618) at the keypoint, mvuRight[i] = x - mbf / d where d > 0,
 * both -1 elsewhere.  depth image b at depth + b * image_stride, rows `stride` floats apart (host memory, or device memory of this GPU).
 * uRight uses mvKeysUn (orbx_set_undistort; mvKeys without distortion), the depth is read at mvKeys, as the reference does.  Results like orbm_stereo_match's: fetch with
 * orbm_stereo_fetch (n_matches = keypoints with a depth), or leave them on the device for orbm_search_local_points_batch.  Asynchronous. */
int orbm_stereo_from_depth(orbx_extractor* h, int first, int B, const float* depth, int stride, size_t image_stride, int depth_on_device, float mbf);

/* Tracking::SearchLocalPoints (src/Tracking.cc:3979-4067 -> Frame::isInFrustum src/Frame.cc:667-773 + ORBmatcher::SearchByProjection
 * src/ORBmatcher.cc:45-167) for a BATCH of frames without leaving the device: frames = images [first, first + B) of the handle's last
 * extraction, read where the extractor left them (mvKeysUn - undistorted on the device when orbx_set_undistort is set -, mDescriptors; mvuRight = the results of
 * orbm_stereo_match / orbm_stereo_from_depth for the same range when use_u_right != 0, else every keypoint is monocular); frames[b] = pose,
 * camera and bounds of frame b (the grid constants are derived from the bounds as Frame does, src/Frame.cc:190-191); the local map is resident
 * (orbm_points); is_bad / has_obs: call-time flags of the M points (NULL = none bad / all observed); occupied: [B][orbx_max_keypoints()] bytes,
 * keypoints that already hold a map point with observations (NULL = none).  The sequential accept loop of the reference (a keypoint that has
 * received a point is skipped by every later point) runs on the device, one wave per frame.  Asynchronous; orbm_search_local_points_fetch
 * returns assigned [B][cap] (index of the map point written to F.mvpMapPoints[i], -1 = untouched), the reference's return value per frame
 * and - when requested here - mbTrackInView [B][M].  ORBX_E_CAPACITY from the fetch = the candidate pool was too small for this scene: it has
 * been enlarged, enqueue the same call again (the refused fetch writes nothing and ends the batch: nothing is pending until then). */
int orbm_search_local_points_batch(orbx_extractor* h, int first, int B, const OrbmFrustumView* frames, const orbm_points* points,
                                   const uint8_t* is_bad, const uint8_t* has_obs, const uint8_t* occupied, int use_u_right,
                                   float viewing_cos_limit, float th, int far_points, float th_far, float nnratio, int want_in_view);
int orbm_search_local_points_fetch(orbx_extractor* h, int* assigned, int cap, int* nmatches, uint8_t* in_view);

/* The same for frames that each bring their OWN local map - independent streams tracked side by side, one frame of every stream per batch.
 * maps[b] is the local map of frame b: a resident set (one set may serve several frames; NULL or an empty set = empty map: the frame gets
 * nmatches = 0 and every assigned entry -1) and that frame's call-time flags over the points of ITS set.  Frame b's results are those of
 * orbm_search_local_points_resident with maps[b]: assigned[b][i] indexes frame b's own set.  Everything else - frames, occupied, the parameters,
 * the one pending batch per handle, the candidate pool (ORBX_E_CAPACITY from the fetch, then enqueue again) - as orbm_search_local_points_batch;
 * also refused (ORBX_E_ARG, nothing enqueued, nothing to fetch): maps == NULL, a set that lives on another device than the handle.
 * orbm_search_local_points_fetch returns mbTrackInView as [B][M_max], M_max = the largest orbm_points_count of the batch: row b holds frame
 * b's M_b flags, then zeros.  (The struct is declared apart from its typedef - the same C type - because tests/test_struct_layout.py keeps a fixed
 * list of the header's `typedef struct X { .. } X;` records; this one's Python mirror is checked by tests/test_local_points_maps.py.) */
struct OrbmFrameMap {
    const orbm_points* points;             /* resident set; one set may serve many frames; NULL or M == 0 = empty map */
    const uint8_t* is_bad;                 /* [M of that set] call-time flags, NULL = none bad */
    const uint8_t* has_obs;                /* [M of that set], NULL = all observed */
};
typedef struct OrbmFrameMap OrbmFrameMap;  /* the local map of ONE frame of a batch */
int orbm_search_local_points_batch_maps(orbx_extractor* h, int first, int B, const OrbmFrustumView* frames, const OrbmFrameMap* maps /*[B]*/,
                                        const uint8_t* occupied, int use_u_right, float viewing_cos_limit, float th, int far_points, float th_far,
                                        float nnratio, int want_in_view);
int orbm_points_count(const orbm_points* p);     /* M of a resident set (0 for NULL) */

/* The map on the device.  A map point's fields change where LocalMapping / LoopClosing touch it, but the LIST a frame is matched against does
 * not change slowly: Tracking::TrackLocalMap calls UpdateLocalMap() for every frame, and Tracking::UpdateLocalPoints (src/Tracking.cc:4088-4120)
 * rebuilds mvpLocalMapPoints from scratch - the local key frames in reverse order, each one's GetMapPointMatches() in feature order, skipping
 * nulls, points already stamped for this frame and bad points.  An orbm_map keeps the fields the searches read in a store addressed by SLOT (the
 * caller's id of a MapPoint, 0 .. slots - 1), the map-point matches of key frames as rows of slots, and builds the list of B frames on the
 * device into ordinary orbm_points sets, in the reference's order (the accept loops depend on it).  Every search that takes an orbm_points
 * takes such a set unchanged.
 *   Sets belong to the map: orbm_points_destroy does nothing to them.  Set b stays valid until the next orbm_map_local_points / orbm_map_select
 * that writes set b, or orbm_map_destroy; a batch that was enqueued on a set and not fetched yet HAS TO BE FETCHED before that set is rebuilt
 * (the set's memory is reused in place, or freed when it has to grow).  Buffers grow to the sizes seen and are reused: no allocation per build.
 *   Every call takes a mutex inside the map and waits for its own work on the stream of the handle it was given, so one map may be updated
 * through LocalMapping's handle and read through Tracking's; any handle of the map's device will do, a handle of another device is ORBX_E_ARG.
 *   Refusals come before anything is enqueued and leave the map as it was: ORBX_E_ARG for null pointers, negative sizes, slots / rows / sets
 * out of range and duplicate slots (the message names the frame, row or entry), ORBX_E_CAPACITY for n > kf_row_cap, B > max_sets and the
 * limits of orbm_map_create (at most 2^28 slots, 65 535 sets, rows of 2^22 features).  Nothing is ever truncated.
 *   Device memory: 65 * slots (store) + 4 * kf_rows * kf_row_cap (rows) + 8 * max_sets * slots (first-occurrence and seen stamps) bytes at
 * creation; each set that has been built holds 69 bytes per point of the largest list it has held; one staging block of about
 * 20 * (rows visited) + 8 * (positions visited) / 256 + 4 * (seen slots) bytes of the largest call (12 bytes per edit of orbm_map_edit_keyframes);
 * 4 * slots more from the first orbm_fuse_candidates_batch_map / orbm_search_by_projection_sim3_batch_map on, for their table by slot - nothing of it
 * at creation.  orbx_debug_live_resources counts all of it. */
typedef struct orbm_map orbm_map;
int orbm_map_create(orbx_extractor* h, int slots, int kf_rows, int kf_row_cap, int max_sets, orbm_map** out);
int orbm_map_destroy(orbx_extractor* h, orbm_map* m);
/* n distinct slots get the fields the searches read (pos, normal, mfMinDistance, mfMaxDistance, descriptor; view->M == n).
 * view->is_bad (NULL = 0) is stored; view->has_obs is ignored.  A slot that was never updated is absent: it behaves as bad and is never emitted. */
int orbm_map_update(orbx_extractor* h, orbm_map* m, int n, const int* slots, const OrbmWorldPointView* view);
/* MapPoint::SetBadFlag (or its reverse) for n distinct slots; an absent slot stays absent */
int orbm_map_set_bad(orbx_extractor* h, orbm_map* m, int n, const int* slots, const uint8_t* bad);
/* GetMapPointMatches() of one key frame: slot of feature i, or -1 */
int orbm_map_set_keyframe(orbx_extractor* h, orbm_map* m, int row, int n, const int* slots);
/* Tracking::UpdateLocalPoints for B frames: frame b visits rows kf_rows[kf_start[b] .. kf_start[b+1]) in THAT order (the caller lists
 * mvpLocalKeyFrames reversed, as the reference walks them).  Position p of the walk keeps its point iff the slot is >= 0, present and not bad
 * and no earlier position of this frame holds the same slot.  seen_* (may be NULL): the slots frame b already holds (SearchLocalPoints'
 * first loop, src/Tracking.cc:3983-4003), seen_slots[seen_start[b] .. seen_start[b+1]); duplicates and slots outside the local map are fine.
 * Result: set b (orbm_map_set), M_out[b] points; orbm_map_set_fetch gives slots[j] = the slot of local point j (the way back from `assigned` to
 * the MapPoint) and seen[j] = 1 iff that slot is in the frame's seen list - hand it to the searches as is_bad (mnLastFrameSeen ==
 * mCurrentFrame.mnId, src/Tracking.cc:4015) and leave has_obs NULL (a good point in a key frame's matches has observations).  Blocking. */
int orbm_map_local_points(orbx_extractor* h, orbm_map* m, int B, const int* kf_start, const int* kf_rows,
                          const int* seen_start, const int* seen_slots, int* M_out);
/* an explicit list (the point set of a Fuse: one key frame's good map points) into set b; slots valid and present, duplicates allowed */
int orbm_map_select(orbx_extractor* h, orbm_map* m, int b, int n, const int* slots);
const orbm_points* orbm_map_set(orbx_extractor* h, const orbm_map* m, int b);      /* owned by the map; NULL for a set that was never built */
int orbm_map_set_fetch(orbx_extractor* h, const orbm_map* m, int b, int* slots /*[M_b]*/, uint8_t* seen /*[M_b]*/);
int orbm_points_fetch(orbx_extractor* h, const orbm_points* p, float* pos, float* normal, float* min_distance, float* max_distance,
                      uint8_t* desc);   /* any may be NULL; works for every orbm_points */
/* tests: the stamp value at which the map's epoch of first-occurrence stamps is used up and the stamps are cleared (0 = the default, 2^32 - 1);
 * a frame that visits more positions than that is ORBX_E_CAPACITY */
int orbm_map_debug_epoch(orbx_extractor* h, orbm_map* m, int limit);

/* ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1950-2184, one camera) - the search of
 * Tracking::TrackWithMotionModel - for a BATCH of frames on the device: current frames = images [first, first + B) of the handle's last
 * extraction (mvKeysUn, mDescriptors, mvuRight as in orbm_search_local_points_batch); cur[b] = pose, camera, bounds, mbf and scale factors of
 * current frame b; `last` = per frame the map points of ITS last frame, cap_last rows per frame: world position, valid
 * (mvpMapPoints[i] != NULL && !mvbOutlier[i]), octave and angle of the last frame's keypoint i, Observations() > 0, descriptor.
 * forward / backward: [B] bytes, bForward / bBackward of each pair of poses (:1973-1975).  Projection, image test, level window, window search,
 * right-coordinate gate, Hamming distances, the sequential accept loop and the rotation histogram with its three maxima all run on the
 * device.  Asynchronous; orbm_search_local_points_fetch returns assigned [B][cap] (index into the last frame's points, -1 untouched, -2 reset
 * to NULL by the rotation check) and the return value per frame.
 * ONE pending batch per handle: orbm_search_local_points_batch and this call share the result block; enqueueing either of them discards a
 * batch that has not been fetched yet, and a call that fails leaves nothing to fetch (orbm_search_local_points_fetch then returns ORBX_E_ARG). */
typedef struct OrbmLastFrameBatch {
    int cap_last;                          /* rows per frame in the arrays below */
    const int* n;                          /* [B] LastFrame.N */
    const float* pos;                      /* [B][cap_last][3] pMP->GetWorldPos() */
    const uint8_t* valid;                  /* [B][cap_last] */
    const int* octave;                     /* [B][cap_last] */
    const float* angle;                    /* [B][cap_last] */
    const uint8_t* has_obs;                /* [B][cap_last] (NULL = all observed) */
    const uint8_t* desc;                   /* [B][cap_last][32] */
} OrbmLastFrameBatch;
int orbm_search_by_projection_lastframe_batch(orbx_extractor* h, int first, int B, const OrbmFrustumView* cur, const OrbmLastFrameBatch* last,
                                              float th, const uint8_t* forward, const uint8_t* backward, int check_orientation,
                                              const uint8_t* occupied, int use_u_right);

/* ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:2196-2324) -
 * the search of Tracking::Relocalization (src/Tracking.cc:4480, :4500) - for a BATCH of frames on the device: current frames = images
 * [first, first + B) of the handle's last extraction, cur[b] = pose (quaternion + translation + mOw), camera, bounds and scale factors of frame b;
 * `kf` = per frame the map points of ITS candidate key frame, cap_kf rows per frame: world position, valid (pMP != NULL && !pMP->isBad() &&
 * !sAlreadyFound.count(pMP)), mfMinDistance / mfMaxDistance (the device applies the 0.8 / 1.2 of Get*DistanceInvariance and evaluates
 * MapPoint::PredictScale(dist3D, &CurrentFrame) itself), the angle of the key frame's keypoint i (pKF->mvKeysUn[i].angle), the descriptor.
 * occupied [B][cap] = CurrentFrame.mvpMapPoints[i] != NULL beforehand (NULL = none).  Projection (Tcw * x3Dw on the quaternion), image test, distance
 * range, predicted level, window search, Hamming distances, the sequential accept loop (best distance <= orb_dist; every accepted point occupies its
 * keypoint) and the rotation histogram run on the device.  Asynchronous; orbm_search_local_points_fetch returns assigned [B][cap] (index into the
 * key frame's rows, -1 untouched, -2 reset by the rotation check) and the return value per frame.  Shares the one pending batch of the handle. */
typedef struct OrbmKeyFramePointBatch {
    int cap_kf;                            /* rows per frame in the arrays below */
    const int* n;                          /* [B] pKF->GetMapPointMatches().size() */
    const float* pos;                      /* [B][cap_kf][3] */
    const uint8_t* valid;                  /* [B][cap_kf] */
    const float* min_distance;             /* [B][cap_kf] mfMinDistance */
    const float* max_distance;             /* [B][cap_kf] mfMaxDistance */
    const float* angle;                    /* [B][cap_kf] */
    const uint8_t* desc;                   /* [B][cap_kf][32] */
} OrbmKeyFramePointBatch;
int orbm_search_by_projection_keyframe_batch(orbx_extractor* h, int first, int B, const OrbmFrustumView* cur, const OrbmKeyFramePointBatch* kf,
                                             float th, int orb_dist, int check_orientation, const uint8_t* occupied);

/* ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) (src/ORBmatcher.cc:1950-2184).
 * forward/backward = bForward/bBackward (:1973-1975, computed from the two poses by the caller).
 * assigned[i] = index into LastFrame of the point written to CurrentFrame.mvpMapPoints[i]; -1 untouched;
 * -2 = written and then reset to NULL by the rotation-consistency check. */
int orbm_search_by_projection_frame(orbx_extractor* h, const OrbmFrameView* Cur, const OrbmLastFrameView* Last,
                                    float th, int forward, int backward, int check_orientation,
                                    int* assigned, int* nmatches);

typedef struct OrbmKeyFrameView {         /* what SearchForTriangulation reads of a KeyFrame, include/KeyFrame.h */
    int N;
    const OrbxKeyPoint* keys_un;          /* mvKeysUn */
    const uint8_t* desc;                  /* mDescriptors */
    const float* u_right;                 /* mvuRight (NULL = all monocular) */
    const uint8_t* has_map_point;         /* GetMapPoint(i) != NULL */
    int fv_nodes;                         /* mFeatVec (DBoW2::FeatureVector = map<NodeId, vector<unsigned>>) as CSR: */
    const uint32_t* fv_node_id;           /*   node ids, ascending */
    const int* fv_start;                  /*   fv_nodes + 1 offsets into fv_feat */
    const uint32_t* fv_feat;              /*   feature indices, in each node's insertion order */
    int nlevels; const float* scale_factors; const float* level_sigma2;
} OrbmKeyFrameView;

/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse) (src/ORBmatcher.cc:1045-1323),
 * pinhole / no second camera.  F12 = K1^-T [t12]x R12 K2^-1 row-major and ep = the epipole, as the reference computes them
 * (:1061-1063, Pinhole.cpp:186-192).  matches12[i] = idx2 matched to feature i of KF1, or -1. */
int orbm_search_for_triangulation(orbx_extractor* h, const OrbmKeyFrameView* K1, const OrbmKeyFrameView* K2,
                                  const float F12[9], const float ep[2], int only_stereo, int coarse,
                                  int check_orientation, int* matches12, int* nmatches);

/* The same for one key frame against n2 neighbours in one launch (LocalMapping::CreateNewMapPoints loops over 10-30 neighbour key frames,
 * src/LocalMapping.cc:510-540): F12s = n2 x 9, eps = n2 x 2, matches12 = n2 rows of K1->N entries, nmatches = n2 counts. */
int orbm_search_for_triangulation_batch(orbx_extractor* h, const OrbmKeyFrameView* K1, int n2, const OrbmKeyFrameView* const* K2s,
                                        const float* F12s, const float* eps, int only_stereo, int coarse, int check_orientation,
                                        int* matches12, int* nmatches);

/* The same for key frames with Kannala-Brandt cameras - one fisheye camera, or a fisheye rig (mpCamera2 != NULL, features [0, NLeft) from
 * camera 1 and [NLeft, N) from camera 2): the epipolar test is KannalaBrandt8::epipolarConstrain = TriangulateMatches > 1e-4
 * (src/CameraModels/KannalaBrandt8.cpp:322-328), with the relative pose chosen per pair of cameras (src/ORBmatcher.cc:1203-1240).
 * K1 / K2->keys_un hold mvKeys followed by mvKeysRight for a rig (mvKeysUn for one camera), u_right = NULL for a rig. */
typedef struct OrbmKB8Pair {
    int nleft1, nleft2;                   /* KeyFrame::NLeft of KF1 / KF2, -1 = one camera */
    float cam1[2][8], cam2[2][8];         /* mvParameters of mpCamera, mpCamera2 of KF1 and of KF2 (the second is ignored for one camera) */
    float R[4][9], t[4][3];               /* [bRight1 * 2 + bRight2]: rotation (row-major) / translation of Tll, Tlr, Trl, Trr (:1067-1083);
                                             one camera: entry 0 = T12 = T1w * Tw2 */
} OrbmKB8Pair;
int orbm_search_for_triangulation_kb8(orbx_extractor* h, const OrbmKeyFrameView* K1, const OrbmKeyFrameView* K2, const OrbmKB8Pair* cams,
                                      const float ep[2], int only_stereo, int coarse, int check_orientation, int* matches12, int* nmatches);

/* Batched Frame::GetFeaturesInArea + Hamming distance: the building block the remaining projection-type searches of the
 * reference (SearchByProjection(KeyFrame*, Sim3, ...) src/ORBmatcher.cc:495-732, SearchByProjection(Frame&, KeyFrame*, ...) :2196-2324,
 * Fuse :1325-1675, SearchBySim3 :1689-1932) share: for every query (x, y, r, minLevel, maxLevel, descriptor) the keypoints
 * of F in the window, in the reference's GetFeaturesInArea order, with their distance to the query descriptor and their octave.
 * None of those callers has an order-dependent accept loop, so they take the minimum over their own gates on these lists.
 * CSR output: start[Q], count[Q]; entry k of query q is idx[start[q]+k], dist[...], level[...].  `cap` = capacity of the entry
 * arrays; returns the total number of entries (> cap: nothing is copied, call again with a larger cap). */
typedef struct OrbmAreaQuery { float x, y, r; int min_level, max_level; } OrbmAreaQuery;
int orbm_area_search_batch(orbx_extractor* h, const OrbmFrameView* F, const OrbmAreaQuery* queries, const uint8_t* query_desc, int Q,
                           int* start, int* count, int* idx, int* dist, int* level, int cap);

/* ---- Input pre-step: what the reference does to a camera frame between the driver and ORBextractor ----
 * geometry 1 = cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR), the stereo rectification of System::TrackStereo (src/System.cc:286-293,
 * maps of cv::initUndistortRectifyMap(..., CV_32F, ...), src/Settings.cc:549-574); geometry 2 = cv::resize(im, imToFeed, newImSize)
 * (src/System.cc:295-297, e.g. 752x480 -> 600x350 in Examples/Monocular/EuRoC.yaml:36-37); then, for 3/4-channel frames,
 * cv::cvtColor(..., COLOR_RGB2GRAY | BGR2GRAY | RGBA2GRAY | BGRA2GRAY) of Tracking::GrabImage* (src/Tracking.cc:1532-1560, rgb = mbRGB).
 * With a spec set, orbx_extract / orbx_extract_batch take the raw frames (width, height, stride of the source, `channels` bytes per
 * pixel) and extract at out_w x out_h (geometry != 0) or at the source size.  NULL restores plain 8UC1 input. */
typedef struct OrbxInputSpec {
    int channels;                        /* 1, 3 or 4 */
    int rgb;                             /* Tracking::mbRGB: 1 = red first, 0 = blue first */
    int gray_variant;                    /* cvtColor 8U coefficients: 0 = OpenCV 4.x (9798, 19235, 3735 >> 15), 1 = 3.x (4899, 9617, 1868 >> 14) */
    int geometry;                        /* 0 none, 1 remap, 2 resize */
    int out_w, out_h;                    /* size fed to the extractor when geometry != 0 (map size / Settings::newImSize()) */
    const float* map_x; const float* map_y;   /* geometry 1: M1, M2 (CV_32FC1, out_h x out_w, dense); copied to the device */
} OrbxInputSpec;
int orbx_set_input(orbx_extractor* h, const OrbxInputSpec* spec);

/* ---- two-camera (fisheye rig, Frame::Nleft != -1) branches of the SearchByProjection overloads ----
 * left  = the view of camera 1: keys_un = mvKeys, desc = descriptor rows [0, Nleft), occupied = mvpMapPoints[0, Nleft) (with observations);
 * right = the view of camera 2: keys_un = mvKeysRight, desc = rows [Nleft, N), occupied = mvpMapPoints[Nleft, N); u_right is not read.
 * Both views carry the frame's bounds / grid parameters (the right grid is mGridRight). */
typedef struct OrbmFisheyeFrameView {
    OrbmFrameView left, right;
    const int* left_to_right;             /* mvLeftToRightMatch [Nleft]  (read by the map-point overload only; NULL = all -1) */
    const int* right_to_left;             /* mvRightToLeftMatch [Nright] (read by the map-point overload only; NULL = all -1) */
} OrbmFisheyeFrameView;
typedef struct OrbmMapPointRightView {    /* the *R tracking fields of MapPoint, include/MapPoint.h:175-179 */
    const uint8_t* in_view_r;             /* mbTrackInViewR */
    const float* proj_xr; const float* proj_yr;   /* mTrackProjXR / mTrackProjYR */
    const int* scale_level_r;             /* mnTrackScaleLevelR (-1 = not set) */
    const float* view_cos_r;              /* mTrackViewCosR */
} OrbmMapPointRightView;
/* ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints) with F.Nleft != -1
 * (src/ORBmatcher.cc:45-239 including :170-236).  assigned has Nleft + Nright entries, indexed like F.mvpMapPoints. */
int orbm_search_by_projection_mappoints_fisheye(orbx_extractor* h, const OrbmFisheyeFrameView* F, const OrbmMapPointView* P,
                                                const OrbmMapPointRightView* PR, float th, int far_points, float th_far_points,
                                                float nnratio, int* assigned, int* nmatches);
/* Frame::isInFrustum for a two-camera rig (Nleft != -1, src/Frame.cc:754-766): Frame::isInFrustumChecks (:1592-1650) once per camera on the
 * device.  `left` = camera 1 as in OrbmFrustumView (mRcw, mtcw, mOw, mpCamera, the image bounds); camera 2 is derived exactly as the reference
 * derives it: mR = Rrl * mRcw, mt = Rrl * mtcw + trl, twc = mRwc * tlr + mOw (Eigen >= 3.3's sums: a0 + (a1 + a2)), projected with mpCamera2.  A point
 * that fails any test of a camera leaves that camera's fields untouched in the reference; here its in-view flag is 0, its level -1 and the
 * other fields unspecified. */
typedef struct OrbmFrustumRigView {
    OrbmFrustumView left;                 /* camera 1 */
    float Rrl[9], trl[3];                 /* mTrl.rotationMatrix() (row-major), mTrl.translation() */
    float tlr[3];                         /* mTlr.translation() */
    float Rwc[9];                         /* mRwc (row-major) */
    int camera2_type; float cam2[8];      /* mpCamera2: GetType(), parameters */
} OrbmFrustumRigView;
typedef struct OrbmTrackOutRight { uint8_t* in_view_r; float *proj_xr, *proj_yr, *depth_r, *view_cos_r; int* scale_level_r; } OrbmTrackOutRight;   /* the *R fields, include/MapPoint.h:175-179 */
int orbm_is_in_frustum_rig(orbx_extractor* h, const OrbmFrustumRigView* frame, const OrbmWorldPointView* points, float viewing_cos_limit,
                           const OrbmTrackOut* left, const OrbmTrackOutRight* right);
/* Tracking::SearchLocalPoints for a rig frame (src/Tracking.cc:3979-4067 with Nleft != -1): the two-camera isInFrustum on the device, then
 * ORBmatcher::SearchByProjection(F, points, th, bFarPoints, thFarPoints) with its right-camera branch (src/ORBmatcher.cc:45-239).  assigned has
 * Nleft + Nright entries; left / right (may be NULL) receive the tracking fields. */
int orbm_search_local_points_fisheye(orbx_extractor* h, const OrbmFisheyeFrameView* F, const OrbmFrustumRigView* frame, const OrbmWorldPointView* points,
                                     float viewing_cos_limit, float th, int far_points, float th_far, float nnratio, const OrbmTrackOut* left,
                                     const OrbmTrackOutRight* right, int* assigned, int* nmatches);
/* ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) with CurrentFrame.Nleft != -1
 * (src/ORBmatcher.cc:1950-2184 including :2090-2150).  proj_ur / proj_vr [Last->N] = project(GetRelativePoseTrl() * x3Dc).
 * assigned has Nleft + Nright entries (-1 untouched, -2 reset by the rotation check). */
int orbm_search_by_projection_frame_fisheye(orbx_extractor* h, const OrbmFisheyeFrameView* Cur, const OrbmLastFrameView* Last,
                                            const float* proj_ur, const float* proj_vr, float th, int forward, int backward,
                                            int check_orientation, int* assigned, int* nmatches);

/* The two searches above for a BATCH of rig frames without leaving the device.  Frame b = left image lf + b of L's last extraction (camera 1:
 * mvKeys, its descriptors) and right image rf + b of R's last extraction (camera 2: mvKeysRight), linked by the mvLeftToRightMatch /
 * mvRightToLeftMatch that the last orbm_stereo_fisheye(L, lf, R, rf, B, ...) left on the device.  L == R is allowed (lf = 0, rf = B for a batch
 * extracted as [L0 .. L(B-1), R0 .. R(B-1)]).  Refused (ORBX_E_ARG) when L has no such orbm_stereo_fisheye call, when that call covered other
 * frames, when either handle has extracted since, when the handles differ in orbx_max_keypoints, levels, scale factor or device.  One grid per
 * camera per frame over the extracted keypoints (not mvKeysUn, as Frame::AssignFeaturesToGrid for Nleft != -1), with the bounds of frames[0]:
 * every frame must have the same bounds.  occupied: [B][2 * orbx_max_keypoints()] bytes in the slot layout of `assigned` (NULL = none).
 * Asynchronous on L's stream; the results are fetched with orbm_search_rig_batch_fetch.  Both calls share L's one pending batch with the
 * single-camera batch searches: any enqueue discards a batch that has not been fetched, and a refused enqueue leaves nothing to fetch. */
/* Tracking::SearchLocalPoints for B rig frames (src/Tracking.cc:3979-4067 with Nleft != -1): per frame the result of
 * orbm_search_local_points_fisheye.  frames[b]: pose (mRcw for the frustum test), cameras and bounds as in orbm_is_in_frustum_rig; the local map
 * is resident; is_bad / has_obs as in orbm_search_local_points_batch. */
int orbm_search_local_points_rig_batch(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const OrbmFrustumRigView* frames,
                                       const orbm_points* points, const uint8_t* is_bad, const uint8_t* has_obs, const uint8_t* occupied,
                                       float viewing_cos_limit, float th, int far_points, float th_far, float nnratio, int want_in_view);
/* The same for rig frames that each bring their own local map (OrbmFrameMap, as orbm_search_local_points_batch_maps): per frame the result of
 * orbm_search_local_points_fisheye with maps[b].  Refused like the call above (no / other / outdated orbm_stereo_fisheye links, differing handles),
 * and for maps == NULL or a set on another device.  orbm_search_rig_batch_fetch returns in_view / in_view_r as [B][M_max], zeros beyond M_b. */
int orbm_search_local_points_rig_batch_maps(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const OrbmFrustumRigView* frames,
                                            const OrbmFrameMap* maps /*[B]*/, const uint8_t* occupied, float viewing_cos_limit, float th, int far_points,
                                            float th_far, float nnratio, int want_in_view);
/* SearchByProjection(CurrentFrame, LastFrame, th, bMono) for B rig frames (src/ORBmatcher.cc:1950-2184 incl. :2089-2152): per frame the result of
 * orbm_search_by_projection_frame_fisheye.  cur[b].left: pose (the quaternion qcw), camera 1 and bounds as in orbm_search_by_projection_lastframe_batch;
 * `last` as there.  Camera 2's projections are made on the device as the reference makes them: x3Dr = CurrentFrame.GetRelativePoseTrl() * x3Dc
 * (Sophus' quaternion action), then CurrentFrame.mpCamera->project(x3Dr) - camera 1's model - and no bounds test.  trl = mTrl: unit quaternion
 * coefficients (x, y, z, w) then the translation, 7 floats for the whole batch. */
int orbm_search_by_projection_lastframe_rig_batch(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const OrbmFrustumRigView* cur,
                                                  const float* trl, const OrbmLastFrameBatch* last, float th, const uint8_t* forward,
                                                  const uint8_t* backward, int check_orientation, const uint8_t* occupied);
/* Results of the last rig batch of L: assigned [B][cap] indexed like F.mvpMapPoints (camera 1 at [0, Nleft), camera 2 at [Nleft, Nleft + Nright);
 * -1 untouched, -2 reset by the rotation check), cap >= 2 * orbx_max_keypoints(); nmatches [B]; in_view / in_view_r [B][M] (mbTrackInView /
 * mbTrackInViewR: local-map form with want_in_view only; after orbm_search_local_points_rig_batch_maps M = M_max, rows padded with zeros).  Every output may be NULL.  ORBX_E_CAPACITY = the candidate pool was too small for
 * this scene: it has been enlarged, enqueue the same call again.  orbm_search_local_points_fetch refuses a rig batch, this call a single-camera one. */
int orbm_search_rig_batch_fetch(orbx_extractor* L, int* assigned, int cap, int* nmatches, uint8_t* in_view, uint8_t* in_view_r);

/* ---- the geometry in front of the projection-type searches, on the device ----
 * SearchByProjection(Frame, LastFrame) (src/ORBmatcher.cc:1993-2010), (Frame, KeyFrame) (:2228-2256), (KeyFrame, Sim3, ...) x2 (:525-560, :640-690),
 * Fuse x2 (:1388-1430, :1590-1625) and SearchBySim3 (:1745-1790, :1830-1875) all start with the same per-map-point chain: transform, depth test,
 * projection, image test, distance range, viewing angle.  orbm_project_points evaluates it for M points at once in the reference's fp32
 * operation order.  The reference multiplies `Tcw * p3Dw` with Sophus types, and Sophus rotates a point by the unit quaternion WITHOUT forming
 * the matrix (Thirdparty/Sophus/sophus/so3.hpp:357-367: uv = 2 q.vec x p; p + q.w uv + q.vec x uv; se3.hpp:321-324 adds the translation;
 * rxso3.hpp:265-273 / sim3.hpp:226-229 for a similarity): poses therefore enter as quaternion coefficients in Eigen's coeffs() order
 * (x, y, z, w) + translation, and the device evaluates exactly those statements (csrc/sophus_action.h; no fused multiply-adds).  R * p + t
 * with R = q.toRotationMatrix() rounds differently in the last bit, which is enough to move a keypoint across a search-window edge.
 * The spec says which tests the method at hand applies and how it writes its projection.  MapPoint::PredictScale stays with the caller's
 * MapPoint (it reads a protected member): `dist` is its argument.  Blocking. */
typedef struct OrbmProjection {
    float q[4], t[3];                     /* p1 = T * p_w: the SE3 pose in front (Tcw, T1w, ...): T.unit_quaternion().coeffs() (x, y, z, w), T.translation() */
    int second; float q2[4], t2[3], s2;   /* a second transform behind it, p_c = X * p1: 0 none; 1 a Sim3 (SearchBySim3's S21 / S12): q2 = X.quaternion().coeffs()
                                           * (not unit: |q2|^2 = scale), t2 = X.translation(), s2 = X.scale(); 2 an SE3 (GetRelativePoseTrl()): unit q2, t2 */
    float Ow[3];                          /* camera centre for the distance / angle tests (dist_mode 0) */
    int dist_mode;                        /* 0: dist = |p_w - Ow|, 1: dist = |p_c| (SearchBySim3, :1771) */
    int depth_test;                       /* 0 none (:2228-2256), 1: p_c.z < 0 rejects, 2: 1 / p_c.z < 0 rejects (:1997-2000) */
    int camera_type; float cam[8];        /* GeometricCamera::GetType(): 0 pinhole (fx, fy, cx, cy), 1 Kannala-Brandt */
    int inline_pinhole;                   /* 1: x = X * (1 / Z), u = fx * x + cx as written out in :656-660 / :1760-1766 instead of mpCamera->project */
    float min_x, max_x, min_y, max_y;     /* mnMinX .. mnMaxY */
    int bounds_mode;                      /* 0: the Frame test (u < min || u > max rejects), 1: KeyFrame::IsInImage (u >= min && u < max), 2: none */
    int distance_test;                    /* dist outside [min_inv, max_inv] rejects */
    int angle_test;                       /* PO . Pn < 0.5 dist rejects (:551, :1416, :1612) */
    float bf;                             /* ur = u - bf / z (Fuse, :1400); 0 otherwise */
} OrbmProjection;
typedef struct OrbmProjectIn {
    int M;
    const float* pos; const float* normal;            /* GetWorldPos(), GetNormal(): M x 3 (normal may be NULL without the angle test) */
    const float* min_inv; const float* max_inv;       /* GetMinDistanceInvariance(), GetMaxDistanceInvariance() (NULL without the distance test) */
    const uint8_t* skip;                              /* 1 = rejected by the caller's own tests (NULL = none) */
} OrbmProjectIn;
typedef struct OrbmProjectOut { uint8_t* valid; float *u, *v, *ur, *inv_z, *dist; } OrbmProjectOut;   /* any array may be NULL */
int orbm_project_points(orbx_extractor* h, const OrbmProjection* spec, const OrbmProjectIn* in, const OrbmProjectOut* out);

/* ---- remaining projection-type searches ----
 * The caller evaluates the geometry in front of GetFeaturesInArea with the reference's own Sophus/Eigen code (Tcw * p3Dw, project,
 * IsInImage, min/max distance, viewing angle, PredictScale) and hands the survivors over as numbers; window search, level window,
 * chi-square gate and every Hamming distance run on the device, the (order-dependent) accept loop is replayed in order. */
typedef struct OrbmProjectedPointView {
    int M;
    const uint8_t* valid;                 /* 1 = the point reaches GetFeaturesInArea in the reference's loop */
    const float* u; const float* v;       /* its projection */
    const float* ur;                      /* uv(0) - bf*invz: read by the Fuse chi-square gate only (may be NULL otherwise) */
    const int* pred_level;                /* pMP->PredictScale(dist, pKF) */
    const float* angle;                   /* pKF->mvKeysUn[i].angle: read by orbm_search_by_projection_keyframe with check_orientation only */
    const uint8_t* desc;                  /* pMP->GetDescriptor(), M x 32 */
} OrbmProjectedPointView;

/* ORBmatcher::SearchByProjection(KeyFrame* pKF, Sim3f& Scw, vpPoints, vpMatched, th, ratioHamming) (src/ORBmatcher.cc:495-606) and
 * the overload that also returns the key frame of each point (:608-732; vpMatchedKF[idx] = vpPointsKFs[assigned[idx]]).
 * KF->occupied[idx] = (vpMatched[idx] != NULL) on entry.  assigned[idx] = index of the point written to vpMatched[idx], else -1. */
int orbm_search_by_projection_sim3(orbx_extractor* h, const OrbmFrameView* KF, const OrbmProjectedPointView* P, float th,
                                   float ratio_hamming, int* assigned, int* nmatches);

/* ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:2196-2324).
 * Cur->occupied[i] = (CurrentFrame.mvpMapPoints[i] != NULL); P has one entry per feature of pKF.  assigned[i] = index into pKF of the
 * map point written to CurrentFrame.mvpMapPoints[i]; -1 untouched; -2 written and reset by the rotation-consistency check. */
int orbm_search_by_projection_keyframe(orbx_extractor* h, const OrbmFrameView* Cur, const OrbmProjectedPointView* P, float th,
                                       int orb_dist, int check_orientation, int* assigned, int* nmatches);

/* Candidate search of ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) (src/ORBmatcher.cc:1325-1528; chi2_gate = 1, inv_level_sigma2 =
 * pKF->mvInvLevelSigma2) and of Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:1543-1660; chi2_gate = 0).  best_idx[i] = the key-frame
 * feature the reference would fuse point i with (bestDist <= TH_LOW), else -1; best_dist may be NULL.  The map surgery that follows
 * (Replace / AddObservation / AddMapPoint) mutates the caller's map and is done by the caller, in point order, from best_idx.
 * For bRight build KF from mvKeysRight / the right descriptors and add NLeft to the returned indices. */
int orbm_fuse_candidates(orbx_extractor* h, const OrbmFrameView* KF, const OrbmProjectedPointView* P, float th, int chi2_gate,
                         const float* inv_level_sigma2, int* best_idx, int* best_dist);

/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, S12, th) (src/ORBmatcher.cc:1689-1932).  P1in2 has one entry per feature of KF1 (its
 * map point transformed by S21 and projected into KF2; valid = present, good, not already matched, passes the depth / image / distance
 * tests), P2in1 the reverse.  matches12[i1] = idx2 of the mutually consistent new match, else -1; *nfound = the reference's return value. */
int orbm_search_by_sim3(orbx_extractor* h, const OrbmFrameView* KF1, const OrbmFrameView* KF2, const OrbmProjectedPointView* P1in2,
                        const OrbmProjectedPointView* P2in1, float th, int* matches12, int* nfound);

/* ---- "next" rows of SURVEY.md §8f, built on the same kernels ---- */
/* ORBmatcher::SearchByBoW.  K1 = the key frame whose map points are searched (has_map_point[i] = map point present and not bad),
 * K2 = the other side.  th_inclusive = 1: SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (src/ORBmatcher.cc:259-493: accept
 * bestDist1 <= TH_LOW, every frame feature is a candidate — K2->has_map_point may be NULL).  th_inclusive = 0:
 * SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (:892-1043: bestDist1 < TH_LOW, only K2 features with a good map point).
 * matches12[i] = index in K2 matched to feature i of K1, or -1 (after the rotation-consistency pruning). */
int orbm_search_by_bow(orbx_extractor* h, const OrbmKeyFrameView* K1, const OrbmKeyFrameView* K2, float nnratio, int th_inclusive,
                       int check_orientation, int* matches12, int* nmatches);

/* n independent (K1s[p], K2s[p]) pairs in one launch: every relocalisation candidate against the current frame (src/Tracking.cc:4360-4380),
 * a key frame against its loop / merge candidates (src/LoopClosing.cc:840-850).  matches12[p] has K1s[p]->N entries, nmatches n entries. */
int orbm_search_by_bow_batch(orbx_extractor* h, int n, const OrbmKeyFrameView* const* K1s, const OrbmKeyFrameView* const* K2s, float nnratio,
                             int th_inclusive, int check_orientation, int* const* matches12, int* nmatches);

/* Device-resident key frames.  What the vocabulary-bucket searches read of a key frame or frame - mvKeysUn, mDescriptors, mvuRight, mFeatVec
 * (include/KeyFrame.h:  the fields of OrbmKeyFrameView) - is uploaded once by orbm_keyframe_create (has_map_point of the view is ignored:
 * map points change while a key frame lives, the searches take the flags per call).  The resident searches give the same results as
 * orbm_search_for_triangulation_batch / orbm_search_by_bow_batch and move only flags, poses and results across the bus; the accept loop of
 * SearchByBoW runs on the device (one wave per vocabulary node).  A key frame may be used with any
 * extractor handle of the device it was created on.  Limit: at most 2048 features of one key frame per vocabulary node (ORBX_E_CAPACITY). */
typedef struct orbm_keyframe orbm_keyframe;
int orbm_keyframe_create(orbx_extractor* h, const OrbmKeyFrameView* K, orbm_keyframe** out);
void orbm_keyframe_destroy(orbm_keyframe* kf);
/* SearchForTriangulation of K1 against n2 neighbours (src/ORBmatcher.cc:1045-1323).  has_map_point1 [K1 N] / has_map_point2[j] [K2s[j] N]:
 * GetMapPoint(i) != NULL at call time (NULL = none).  Other arguments and results as orbm_search_for_triangulation_batch. */
int orbm_search_for_triangulation_resident(orbx_extractor* h, orbm_keyframe* K1, const uint8_t* has_map_point1, int n2, orbm_keyframe* const* K2s,
                                           const uint8_t* const* has_map_point2, const float* F12s, const float* eps, int only_stereo, int coarse,
                                           int check_orientation, int* matches12, int* nmatches);
/* The same for key frames with Kannala-Brandt cameras (one fisheye camera or the rig; the views given to orbm_keyframe_create list mvKeys followed
 * by mvKeysRight and no u_right for a rig, as for orbm_search_for_triangulation_kb8): cams[j] describes the pair (K1, K2s[j]). */
int orbm_search_for_triangulation_resident_kb8(orbx_extractor* h, orbm_keyframe* K1, const uint8_t* has_map_point1, int n2, orbm_keyframe* const* K2s,
                                               const uint8_t* const* has_map_point2, const OrbmKB8Pair* cams, const float* eps, int only_stereo, int coarse,
                                               int check_orientation, int* matches12, int* nmatches);
/* SearchByBoW for n pairs (src/ORBmatcher.cc:259-493, :892-1043).  has_map_point1[p]: K1s[p] features with a good map point (NULL = none, no
 * matches); eligible2[p]: K2s[p] features that may be matched (NULL = all: the Frame overload).  Results as orbm_search_by_bow_batch. */
int orbm_search_by_bow_resident(orbx_extractor* h, int n, orbm_keyframe* const* K1s, const uint8_t* const* has_map_point1, orbm_keyframe* const* K2s,
                                const uint8_t* const* eligible2, float nnratio, int th_inclusive, int check_orientation, int* const* matches12,
                                int* nmatches);

/* The candidate search of ORBmatcher::Fuse for ONE resident point set against K resident key frames in one launch chain: LocalMapping::SearchInNeighbors
 * fuses the current key frame's map points into each of its 20-60 neighbours (src/LocalMapping.cc:999-1040), LoopClosing::SearchAndFuse the loop map points
 * into every key frame of the corrected map (src/LoopClosing.cc:2700-2765).  The search of a (point, key frame) pair reads nothing that the map surgery
 * between two key frames changes - the point's position, normal, distance limits and descriptor, the key frame's pose, camera, keypoints and mvuRight - so
 * all K x M searches run at once; what the surgery does change (isBad, IsInKeyFrame, the key frame's map points) the caller tests when it replays the results,
 * key frame by key frame and point by point, as for the single call.  Target k: `kf` = the resident keypoints / descriptors / mvuRight of ONE camera (for a
 * camera of a rig: a resident key frame made from that camera's keypoints and descriptor rows; add NLeft to the right camera's indices), `spec` = exactly what
 * orbm_project_points takes for Fuse (pose, Ow, camera, bounds, tests, bf), log_scale_factor = pKF->mfLogScaleFactor, inv_level_sigma2 = pKF->mvInvLevelSigma2
 * (as many levels as kf has; read with chi2_gate only).  The device applies the 0.8 / 1.2 of Get*DistanceInvariance to the set's mfMinDistance / mfMaxDistance and
 * evaluates MapPoint::PredictScale(dist3D, pKF) itself (glibc's logf, float division, ceil, the clamps), with the scale factors and level count of `kf`.  The grid
 * of a key frame is built from the spec's bounds (src/Frame.cc:190-191) on its first use and kept inside the orbm_keyframe, keyed by those bounds, until
 * orbm_keyframe_destroy: a covisibility window that comes back pays for it once.
 * skip: [K][M] bytes, pairs the caller already excludes (NULL = none).  chi2_gate = 1: Fuse(pKF, vpMapPoints, th, bRight); 0: Fuse(pKF, Scw, vpPoints, th, ..).
 * best_idx[k][i] / best_dist[k][i] (best_dist may be NULL): as orbm_fuse_candidates gives them for target k - the feature the reference would fuse point i with
 * and its distance, -1 where the pair is skipped, the geometry rejects it or bestDist > TH_LOW; a target without keypoints gives a row of -1.  Blocking.
 * K == 0 or an empty set: ORBX_OK, nothing is written.  Refused before anything is enqueued (ORBX_E_ARG, the message names the target): null arguments,
 * K < 0, a key frame or the point set on another device than the handle, chi2_gate without inv_level_sigma2, a key frame without scale levels.
 * Limits: K <= 65535 and K x M <= 2^28 pairs (ORBX_E_CAPACITY beyond; nothing is truncated).
 * (declared apart from its typedef like OrbmFrameMap; the Python mirror is checked by tests/test_fuse_batch.py) */
struct OrbmFuseTarget {
    const orbm_keyframe* kf;
    OrbmProjection spec;
    float log_scale_factor;
    const float* inv_level_sigma2;
};
typedef struct OrbmFuseTarget OrbmFuseTarget;  /* ONE key frame (one camera) a point set is fused into */
int orbm_fuse_candidates_batch(orbx_extractor* h, int K, const OrbmFuseTarget* targets, const orbm_points* points, const uint8_t* skip /* [K][M] or NULL */,
                               float th, int chi2_gate, int* best_idx /* [K][M] */, int* best_dist /* [K][M] or NULL */);

/* The same search, answered with the matched pairs alone: the replay reads only the pairs with best_idx >= 0, a few per cent of K x M at LoopClosing's
 * shapes, and the dense arrays are most of what the dense call brings down.  The list holds EXACTLY the pairs (k, i) for which orbm_fuse_candidates_batch
 * with the same arguments gives best_idx[k][i] >= 0 (the search kernels are that call's; the list is compacted from its dense result on the device),
 * ordered by k, then by i - the order the replay visits them in (src/ORBmatcher.cc:1494-1520, :1640-1656).  Target k owns entries [start[k], start[k+1]),
 * start[0] = 0; entry e: point[e] = i (the position in the set), feat[e] = best_idx[k][i], dist[e] = best_dist[k][i] (dist may be NULL).  A target without
 * keypoints has an empty span.
 *   Capacity: `cap` = the entries point / feat / dist have room for.  start[0 .. K] is written whenever the call returns ORBX_OK or ORBX_E_CAPACITY.  If
 * start[K] > cap the call returns ORBX_E_CAPACITY and point / feat / dist are untouched - nothing is truncated; call again with cap >= start[K]
 * (cap = K x M always suffices; device memory grows with min(cap, K x M) records, so a tight cap is the cheaper one).  K == 0 or an empty set: ORBX_OK,
 * start all zero, nothing else written.
 *   Blocking.  `start` comes down first and, in the same copy, as many entries as a quarter more than the handle's previous such call found (at least
 * 1024): a list that short costs one wait for the stream, a longer one a second copy of exactly the entries still missing.
 *   Refusals, limits, locking and the grid cache are orbm_fuse_candidates_batch's; refused as well (ORBX_E_ARG, before anything is enqueued): cap < 0, a
 * null start, a null point or feat with cap > 0.  Device memory: the handle's reused scratch (the dense result stays on the device, plus 8 bytes per
 * 256 positions of a target and the records), counted by orbx_debug_live_resources. */
int orbm_fuse_pairs_batch(orbx_extractor* h, int K, const OrbmFuseTarget* targets, const orbm_points* points, const uint8_t* skip /* [K][M] or NULL */,
                          float th, int chi2_gate, int cap, int* start /* [K+1] */, int* point /* [cap] */, int* feat /* [cap] */,
                          int* dist /* [cap] or NULL */);

/* ORBmatcher::SearchByProjection(KeyFrame* pKF, Sim3f& Scw, vpPoints, vpMatched, th, ratioHamming) and the overload that also returns the points' key frames
 * (src/ORBmatcher.cc:495-606, :608-732) for ONE resident point set searched from K resident key frames, each under its own Sim3, in one call: LoopClosing's
 * FindMatchesByProjection searches the matched key frame's covisibility window from the current key frame and DetectCommonRegionsFromBoW searches the same set
 * again from up to five covisible key frames (src/LoopClosing.cc:1046-1090, :1168-1268), for every loop and merge candidate.  The targets are independent of one
 * another (nothing is written to the map between them); INSIDE a target the reference's loop over the points is sequential - a keypoint occupied on entry or
 * taken by an earlier point is invisible to every later point, a point whose best distance is above TH_LOW * ratioHamming takes nothing - and the device
 * reproduces exactly that order.  Target k: `kf` and `spec` as for orbm_fuse_candidates_batch - spec = what orbm_project_points takes for this search: the rigid
 * part [R | t / s] of Scw, Ow = its inverse's translation, the camera (inline_pinhole = 1 for the :608 overload), KeyFrame::IsInImage bounds, depth_test = 1,
 * distance_test = 1, angle_test = 1, bf = 0; log_scale_factor = pKF->mfLogScaleFactor; occupied = [kf N] bytes, vpMatched[idx] != NULL on entry (NULL = none).
 * The device applies the 0.8 / 1.2 of Get*DistanceInvariance and evaluates MapPoint::PredictScale as orbm_fuse_candidates_batch does; the grids are the same
 * per-key-frame cache.  skip: [K][M] bytes, the caller's own exclusions (isBad(), membership in spAlreadyFound; NULL = none).
 * assigned[k][idx] (rows of `cap` entries, cap >= the largest N): the index into the point set of the point the reference writes to vpMatched[idx] of target
 * k, -1 for untouched entries and for the entries from N_k up to cap; nmatches[k]: the reference's return value.  Blocking.
 * K == 0 or an empty set: ORBX_OK, nothing is written.  Refused before anything is enqueued (ORBX_E_ARG, the message names the target): null arguments, K < 0, a
 * key frame or the point set on another device than the handle, empty image bounds, a key frame without scale levels, cap below the largest N.
 * Limits: K <= 65535, K x M <= 2^28 pairs and K x cap <= 2^28 result entries (ORBX_E_CAPACITY beyond; nothing is truncated).
 * (declared apart from its typedef like OrbmFuseTarget; the Python mirror is checked by tests/test_sim3_projection_batch.py) */
struct OrbmSim3Target {
    const orbm_keyframe* kf;
    OrbmProjection spec;
    float log_scale_factor;
    const uint8_t* occupied;
};
typedef struct OrbmSim3Target OrbmSim3Target;  /* ONE (key frame, Sim3) a point set is searched from */
int orbm_search_by_projection_sim3_batch(orbx_extractor* h, int K, const OrbmSim3Target* targets, const orbm_points* points, const uint8_t* skip /* [K][M] or NULL */,
                                         float th, float ratio_hamming, int cap, int* assigned /* [K][cap] */, int* nmatches /* [K] */);

/* SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) for a fisheye-rig frame (F.Nleft != -1; src/ORBmatcher.cc:259-493 incl. :343-372, :414-446).
 * K1 / K2 list ALL features by index (camera 1 first: keys = mvKeys followed by mvKeysRight, descriptor rows as stored); nleft2 = F.Nleft.
 * assigned2[j] = feature of K1 whose map point is written to vpMapPointMatches[j], -1 = NULL (after the rotation-consistency pruning). */
int orbm_search_by_bow_fisheye(orbx_extractor* h, const OrbmKeyFrameView* K1, const OrbmKeyFrameView* K2, int nleft2, float nnratio,
                               int check_orientation, int* assigned2, int* nmatches);

/* ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (src/ORBmatcher.cc:734-880).
 * prev_matched: N1 x 2 floats (vbPrevMatched), updated in place like the reference does (:876-878). */
int orbm_search_for_initialization(orbx_extractor* h, const OrbmFrameView* F1, const OrbmFrameView* F2, float* prev_matched,
                                   int window_size, float nnratio, int check_orientation, int* matches12, int* nmatches);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:438-529) for P map points at once.  Point p owns the
 * descriptors desc[32*start[p] .. 32*start[p+1]) — its observations' descriptors in the reference's iteration order (:451-470).
 * best[p] = index, relative to start[p], of the descriptor the reference would keep (smallest median distance to the others, first on
 * ties); -1 for a point without descriptors. */
int orbm_distinctive_descriptors(orbx_extractor* h, const uint8_t* desc, const int* start, int P, int* best);

/* The same choice with the observations NAMED instead of copied: observation o is row obs_feat[o] of the descriptors of resident key frame
 * kfs[obs_kf[o]] (for a rig key frame the view lists the left camera's features first, so the reference's rightIndex is used as it is).  Point p owns
 * observations [obs_start[p], obs_start[p+1]), in the order the reference pushes them into vDescriptors (its std::map iteration, left index before
 * right index, bad key frames left out by the caller).  best[p] as above (-1: no observations); best_desc row p = the chosen descriptor (untouched for
 * -1; may be NULL).  With map and slots given and slots[p] >= 0 the chosen descriptor also overwrites the descriptor of that slot in the map's store,
 * on the device; a point with best[p] == -1 leaves its slot as it is (the reference returns before assigning mDescriptor), no other field of any slot
 * changes, and sets built earlier keep what they hold (as after orbm_map_update).  New points call with map = NULL or slot -1 and make their first
 * orbm_map_update with the descriptor from best_desc.
 *   Refused before anything is enqueued, the store untouched, the message naming the point or observation: ORBX_E_ARG for null / negative arguments,
 * obs_start decreasing, obs_kf outside [0, nkf), a null key frame, obs_feat outside its key frame's features, a key frame or the map on another device
 * than h, a slot outside the map or holding no point, two points writing one slot; ORBX_E_CAPACITY for more than 1024 observations of one point (nothing
 * is truncated).  P == 0 is ORBX_OK.  Takes the map's mutex like every orbm_map_* call; blocking, on h's stream; staged through h's reused buffers. */
int orbm_distinctive_descriptors_resident(orbx_extractor* h, int nkf, orbm_keyframe* const* kfs, int P, const int* obs_start /*[P+1]*/,
                                          const int* obs_kf /*[total]*/, const int* obs_feat /*[total]*/, orbm_map* map /* may be NULL */,
                                          const int* slots /*[P], may be NULL; -1 = do not write this point*/, int* best /*[P]*/,
                                          uint8_t* best_desc /*[P][32], may be NULL*/);

/* ---- Vocabulary: the consumer right behind the extractor, Frame::ComputeBoW (src/Frame.cc:984-997) ->
 * ORBVocabulary::transform(features, mBowVec, mFeatVec, 4) (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1195).  Produces the
 * FeatureVector CSR that OrbmKeyFrameView (SearchByBoW / SearchForTriangulation) consumes.
 *   Threads: one vocabulary serves every handle of its device, from any thread (Frame::ComputeBoW on Tracking's thread and KeyFrame::ComputeBoW on
 * LocalMapping's share one ORBVocabulary).  It has ONE scratch and ONE set of results; every orbv_* call that touches them, and the two
 * orbm_search_by_bow_*_batch, hold the vocabulary's lock from start to end.  So:
 *   - the blocking orbv_transform is safe from any number of threads at once, each with a handle of its own;
 *   - the split protocol (orbv_transform_extracted / orbv_transform_rig_extracted, later orbv_fetch, orbv_db_add_extracted, orbv_db_query_extracted or
 *     a search batch) has one client at a time: the results belong to the handle (L of a rig run) and extraction that made them until the NEXT run of any
 *     kind on the vocabulary, through any handle.  After that the calls that read them return ORBX_E_ARG ("... were overwritten ...") - never another
 *     run's vectors; transform again.  orbv_fetch right behind a blocking orbv_transform through the same handle keeps working;
 *   - a run through another handle than the previous split-protocol run waits, on the device, until that run has finished (and on the host when it has to
 *     grow the scratch); a run through the same handle is ordered by its stream alone.
 * orbv_destroy must not run beside another call on the same vocabulary. ---- */
typedef struct orbv_vocabulary orbv_vocabulary;

/* Vocabulary from flat arrays in ORBvoc.txt line order (loadFromTextFile, TemplatedVocabulary.h:1338-1430): entry i describes node
 * i + 1; parent[i] (0 = root) must be an earlier node; is_leaf[i] = the file's leaf flag (word ids are handed out to flagged nodes in
 * line order); desc[32*i..]; weight[i].  scoring / weighting = DBoW2::ScoringType / WeightingType (BowVector.h:37-56).
 * The vocabulary lives on h's device. */
int orbv_create(orbx_extractor* h, int k, int L, int scoring, int weighting, int n_nodes, const int* parent, const uint8_t* is_leaf,
                const uint8_t* desc, const double* weight, orbv_vocabulary** out);
/* ORBVocabulary::loadFromTextFile(path) */
int orbv_load_text(orbx_extractor* h, const char* path, orbv_vocabulary** out);
void orbv_destroy(orbv_vocabulary* v);
int orbv_words(const orbv_vocabulary* v);                                       /* ORBVocabulary::size() */

/* transform(features, BowVector&, FeatureVector&, levelsup) for n host descriptors (n x 32).  Any output pointer may be NULL.
 * word_id/node_id [n]: per-feature word and ancestor at level L - levelsup (transform(feature, id, weight, &nid, levelsup), :1218-1259).
 * One case differs from the reference by necessity: a word whose leaf lies ABOVE level L - levelsup (a ragged vocabulary) leaves the reference's `nid` an
 * uninitialised local (:1150, undefined); here the node is then the leaf itself.  ORBvoc.txt at levelsup = 4 has no such leaf.
 * BowVector: bow_id/bow_val (capacity n), ascending word ids, *n_bow entries.  FeatureVector as CSR: fv_node (capacity n, ascending),
 * fv_start (capacity n + 1), fv_feat (capacity n; feature indices in insertion order), *n_fv nodes. */
int orbv_transform(orbv_vocabulary* v, orbx_extractor* h, const uint8_t* desc, int n, int levelsup, uint32_t* word_id, uint32_t* node_id,
                   uint32_t* bow_id, double* bow_val, int* n_bow, uint32_t* fv_node, int* fv_start, uint32_t* fv_feat, int* n_fv);
/* The same for images [first, first + B) of h's last orbx_extract_batch, on the descriptors that are still on the device (no copy);
 * asynchronous on h's stream.  orbv_fetch copies the vectors of image b (relative to `first`) out; capacities = orbx_max_keypoints(h). */
int orbv_transform_extracted(orbv_vocabulary* v, orbx_extractor* h, int first, int B, int levelsup);
int orbv_fetch(orbv_vocabulary* v, orbx_extractor* h, int b, uint32_t* word_id, uint32_t* node_id, int n_features, uint32_t* bow_id, double* bow_val,
               int* n_bow, uint32_t* fv_node, int* fv_start, uint32_t* fv_feat, int* n_fv);

/* Resident key frames made ON THE DEVICE from frames of the handle's last extraction (Tracking::CreateNewKeyFrame for frames that never left the
 * device): out[j] = a key frame of image frames[j] - mvKeysUn (undistorted when the extraction ran with orbx_set_undistort), its descriptor rows,
 * mvuRight = the results of orbm_stereo_match / orbm_stereo_from_depth for that image when use_u_right != 0 (they must cover it, on this extraction), else
 * every entry -1, the FeatureVector where the last orbv_transform_extracted(v, h, first, B, levelsup) left it (frames[j] in [first, first + B)), the
 * handle's scale and sigma tables.  v == NULL: key frames without a FeatureVector (fv_nodes = 0) of any image of the last extraction - what Fuse, the
 * Sim3 projection batch and the per-camera key frames of a rig need.  An index may appear more than once; every occurrence is an object of its own.
 * The key frames are copies with the device layout of orbm_keyframe_create: the next extraction, the vocabulary's next run and orbx_destroy of the
 * handle leave them intact, every resident search takes them through any handle of the device, orbm_keyframe_destroy frees them.  One small block (the
 * frames' sizes) and the keypoint angles come down, nothing goes up but the table of the call.  Blocking.  n == 0: ORBX_OK, nothing is written.
 * Refused before anything is enqueued (ORBX_E_ARG; no object is left behind, out is untouched): null arguments, n < 0, nothing extracted yet, an
 * index outside the extraction or outside the transform's range, a transform of another handle or extraction or one whose results were overwritten,
 * a rig transform, orbx_set_undistort since the extraction, the vocabulary on another device, use_u_right without stereo results for the image. */
int orbm_keyframe_create_extracted(orbx_extractor* h, const orbv_vocabulary* v, int n, const int* frames /*[n]*/, int use_u_right,
                                   orbm_keyframe** out /*[n]*/);
/* The same for rig frames, in the layout orbm_search_for_triangulation_resident_kb8 and orbm_search_by_bow_rig_batch expect: mvKeys of camera 1
 * (not undistorted) followed by mvKeysRight, the joined descriptor rows and the FeatureVector of the last
 * orbv_transform_rig_extracted(v, L, lf, R, rf, B, levelsup), no u_right.  frames[j] in [0, B) names a rig frame as orbm_search_by_bow_rig_batch
 * does.  v is required; a one-camera transform is refused. */
int orbm_keyframe_create_rig_extracted(orbx_extractor* L, int lf, orbx_extractor* R, int rf, const orbv_vocabulary* v, int n,
                                       const int* frames /*[n]*/, orbm_keyframe** out /*[n]*/);
/* Reads a resident key frame back, however it was made.  Any pointer may be NULL; capacities: keys_un, desc (32 B rows), u_right and node_of_feat N,
 * fv_node fv_nodes, fv_start fv_nodes + 1, fv_feat fv_start[fv_nodes] entries (at most N) - a first call with only N / fv_nodes gives the sizes.
 * node_of_feat[f] = index of the node that holds feature f, -1 for a feature in none.  Blocking. */
int orbm_keyframe_fetch(orbx_extractor* h, const orbm_keyframe* kf, int* N, int* fv_nodes, OrbxKeyPoint* keys_un, uint8_t* desc, float* u_right,
                        uint32_t* fv_node, int* fv_start, uint32_t* fv_feat, int* node_of_feat);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches) (src/ORBmatcher.cc:259-493; Tracking::TrackReferenceKeyFrame
 * src/Tracking.cc:3183, Relocalization :4371) for a BATCH of frames on the device: frame b = image first + b of h's last extraction, whose
 * FeatureVector is read where orbv_transform_extracted(v, h, first, B, levelsup) left it (call that first, on the same images); KFs[b] = the
 * device-resident key frame it is searched against (one key frame may serve many frames); has_map_point[b] [KFs[b]->N] = its features with a good
 * map point.  The accept loop per vocabulary node, the ratio and TH_LOW tests and the rotation histogram with its three maxima run on the device
 * (two launches per batch).  matches12[b][i] = frame feature matched to key-frame feature i, or -1, i.e. vpMapPointMatches[matches12[b][i]] =
 * the key frame's map point i; nmatches[b] = the reference's return value.  Blocking. */
int orbm_search_by_bow_frames_batch(orbx_extractor* h, const orbv_vocabulary* v, int first, int B, orbm_keyframe* const* KFs,
                                    const uint8_t* const* has_map_point, float nnratio, int check_orientation, int* const* matches12, int* nmatches);

/* The tracking searches fed from the resident map.  A caller that keeps its map in an orbm_map names the points of the three searches around
 * SearchLocalPoints by SLOT or by key-frame ROW, and the device gathers the fields (k_map_rows_gather, k_map_row_flags) into the block the host-fed
 * calls upload - everything behind that gather is the host-fed call's own code, so results, the fetch calls, the one pending batch per handle and the
 * candidate-pool protocol (ORBX_E_CAPACITY from the fetch, then enqueue again) are those of orbm_search_by_projection_lastframe_batch,
 * .._lastframe_rig_batch, .._keyframe_batch and orbm_search_by_bow_frames_batch.  "The slot holds a point" (orbm_map_update has written it) stands for
 * pMP != NULL; a slot that holds nothing counts as no map point.
 *   Last frame (TrackWithMotionModel; src/ORBmatcher.cc:1981-1983 tests pMP and mvbOutlier[i] only): row i of frame b is used iff i < n[b],
 * slots[b][i] >= 0, the slot holds a point and outlier[b][i] is 0.  The slot's BAD FLAG IS NOT READ: the reference does not call isBad() here and
 * orbm_map_set_bad leaves the fields in place.  Position and descriptor come from the store; octave, angle and has_obs stay host rows - they belong to
 * the last frame's keypoints and to the tracker (a temporal point of UpdateLastFrame gets a slot by orbm_map_update like any point, with has_obs = 0).
 * A slot may appear many times in a row.
 *   Key frame (Relocalization; :2218-2220): row i is used iff i is below the length of row[b], its slot is >= 0 and holds a point that is NOT bad, and
 * found[b][i] is 0.  Position, mfMinDistance, mfMaxDistance and descriptor come from the store, the angle from keypoint i of kfs[b]
 * (pKF->mvKeysUn[i].angle); the row's length and kfs[b]'s N have to be equal.  assigned indexes the row.
 *   BoW (TrackReferenceKeyFrame, Relocalization): has_map_point[b][i] = the key-frame rule without `found`, for row rows[b] and key frame KFs[b].
 *   The map: results equal a gather at the moment of the call, whatever any handle does to the map afterwards.  Each call takes the map's mutex,
 * enqueues upload and gather, waits on the host for an event recorded right behind the gather - for that only, not for the search - and releases the
 * mutex; the search stays asynchronous.  orbm_search_by_bow_frames_batch_map is blocking as its host-fed form and holds the vocabulary's lock and the
 * map's mutex, taken in that order.  The key frames kfs[b] / KFs[b] are read by the gather too and may be destroyed once the call has returned
 * (projection forms; the BoW search has ended by then).
 *   Refusals come before anything is enqueued, leave nothing to fetch and name frame and entry: ORBX_E_ARG for a null map, last, kf, rows or KFs, a
 * map on another device than the handle, n[b] outside [0, cap_last], a used slot below -1 or at or above the map's slots, a row outside the map or
 * never set (orbm_map_set_keyframe), a row length other than kfs[b]'s N, found != NULL with cap_found below a used row's length, and everything the
 * host-fed calls refuse; ORBX_E_CAPACITY as theirs (LDS of the accept kernel: cap_last, or the longest row).  Device memory: the handle's batch
 * block as for the host-fed calls (the gathered rows take the place of the uploaded ones); orbx_debug_live_resources counts it.
 * (The structs are declared apart from their typedefs like OrbmFrameMap; their Python mirrors are checked by tests/test_map_rows_projection.py.) */
struct OrbmLastFrameSlots {            /* LastFrame.mvpMapPoints as slots of an orbm_map */
    int cap_last;                      /* entries per frame in the arrays below */
    const int* n;                      /* [B] LastFrame.N */
    const int* slots;                  /* [B][cap_last] slot of mvpMapPoints[i], -1 = NULL */
    const uint8_t* outlier;            /* [B][cap_last] LastFrame.mvbOutlier[i] (NULL = none) */
    const int* octave;                 /* [B][cap_last] as OrbmLastFrameBatch */
    const float* angle;                /* [B][cap_last] as OrbmLastFrameBatch */
    const uint8_t* has_obs;            /* [B][cap_last] (NULL = all observed) */
};
typedef struct OrbmLastFrameSlots OrbmLastFrameSlots;
int orbm_search_by_projection_lastframe_batch_map(orbx_extractor* h, int first, int B, const OrbmFrustumView* cur, orbm_map* map,
                                                  const OrbmLastFrameSlots* last, float th, const uint8_t* forward, const uint8_t* backward,
                                                  int check_orientation, const uint8_t* occupied, int use_u_right);
int orbm_search_by_projection_lastframe_rig_batch_map(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const OrbmFrustumRigView* cur,
                                                      const float* trl, orbm_map* map, const OrbmLastFrameSlots* last, float th,
                                                      const uint8_t* forward, const uint8_t* backward, int check_orientation, const uint8_t* occupied);
struct OrbmKeyFrameRows {              /* the candidate key frame of each frame, by its place in the map */
    const int* row;                    /* [B] the key frame's row (orbm_map_set_keyframe) */
    orbm_keyframe* const* kfs;         /* [B] the same key frame, resident: pKF->mvKeysUn[i].angle is read from it */
    int cap_found;                     /* entries per frame of `found` */
    const uint8_t* found;              /* [B][cap_found] sAlreadyFound.count(vpMPs[i]) (NULL = none found) */
};
typedef struct OrbmKeyFrameRows OrbmKeyFrameRows;
int orbm_search_by_projection_keyframe_batch_map(orbx_extractor* h, int first, int B, const OrbmFrustumView* cur, orbm_map* map,
                                                 const OrbmKeyFrameRows* kf, float th, int orb_dist, int check_orientation, const uint8_t* occupied);
int orbm_search_by_bow_frames_batch_map(orbx_extractor* h, const orbv_vocabulary* v, int first, int B, orbm_keyframe* const* KFs, orbm_map* map,
                                        const int* rows /*[B]*/, float nnratio, int check_orientation, int* const* matches12, int* nmatches);

/* The resident key-frame searches with their call-time flags read from the map: each flag array of the host-fed call is named by the ROW of its
 * key frame (orbm_map_set_keyframe) and filled on the device from the row's slots and the slots' states, all arrays of a call in one launch.
 * Everything else - arguments, results, limits - as orbm_search_for_triangulation_resident[_kb8], orbm_search_by_bow_resident and
 * orbm_search_by_bow_rig_batch.  Two rules, as the reference has them:
 *   holds a point (slot >= 0 and the slot holds a point; the BAD FLAG IS NOT READ - src/ORBmatcher.cc:1123-1127 and :1159-1163 test the pointer
 * only): has_map_point1 (row1) and has_map_point2 (rows2[j]) of both triangulation searches;
 *   holds a good point (slot >= 0, holds a point, not bad - `!pMP || pMP->isBad()`, :938-941, :959-965, :306-312): has_map_point1 (rows1[p]) and
 * eligible2 (rows2[p]; rows2 == NULL or rows2[p] == -1: every feature of K2s[p] is eligible) of orbm_search_by_bow_resident_map, has_map_point
 * (rows[p]) of orbm_search_by_bow_rig_batch_map.
 *   Blocking like the host-fed forms; the map's mutex is held until the call returns, orbm_search_by_bow_rig_batch_map takes the vocabulary's
 * lock first.  Refused with ORBX_E_ARG before anything is enqueued: a null map or row list, a map on another device than the handle, a row
 * outside the map or never set, a row whose length is not its key frame's N, and everything the host-fed calls refuse. */
int orbm_search_for_triangulation_resident_map(orbx_extractor* h, orbm_keyframe* K1, int row1, int n2, orbm_keyframe* const* K2s,
                                               const int* rows2 /*[n2]*/, orbm_map* map, const float* F12s, const float* eps, int only_stereo,
                                               int coarse, int check_orientation, int* matches12, int* nmatches);
int orbm_search_for_triangulation_resident_kb8_map(orbx_extractor* h, orbm_keyframe* K1, int row1, int n2, orbm_keyframe* const* K2s,
                                                   const int* rows2 /*[n2]*/, orbm_map* map, const OrbmKB8Pair* cams, const float* eps,
                                                   int only_stereo, int coarse, int check_orientation, int* matches12, int* nmatches);
int orbm_search_by_bow_resident_map(orbx_extractor* h, int n, orbm_keyframe* const* K1s, const int* rows1 /*[n]*/, orbm_keyframe* const* K2s,
                                    const int* rows2 /*[n] or NULL*/, orbm_map* map, float nnratio, int th_inclusive, int check_orientation,
                                    int* const* matches12, int* nmatches);
int orbm_search_by_bow_rig_batch_map(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const orbv_vocabulary* v, int P, const int* frame,
                                     orbm_keyframe* const* KFs, orbm_map* map, const int* rows /*[P]*/, float nnratio, int check_orientation,
                                     int* const* assigned, int* nmatches);

/* Tracking::SearchLocalPoints on the map's OWN sets: frame b is searched against set set0 + b of `map` as the last orbm_map_local_points /
 * orbm_map_select left it, and nothing per point crosses the bus in either direction.  is_bad of frame b = the `seen` bytes of its set, read on the
 * device (a selected set has seen = 0); has_obs = all observed.  Per frame the result equals orbm_search_local_points_batch_maps /
 * orbm_search_local_points_rig_batch_maps given {orbm_map_set(set0 + b), the seen bytes orbm_map_set_fetch returns, NULL}; a set that was never
 * built or is empty gives nmatches 0 and every entry -1.  Everything else - frames, occupied, the parameters, the one pending batch per handle,
 * the candidate pool (ORBX_E_CAPACITY from the fetch, then enqueue again), want_in_view - as those calls.
 *   orbm_search_local_points_fetch_slots / orbm_search_rig_batch_fetch_slots: as orbm_search_local_points_fetch / orbm_search_rig_batch_fetch, but
 * assigned_slot[b][i] is the map SLOT of the point written to keypoint i (both cameras' halves of a rig row), translated on the device behind
 * the accept loop; negative entries pass through.  Valid only for a pending batch enqueued by one of the two calls here: on any other pending
 * batch they return ORBX_E_ARG and leave it pending.  The plain fetches keep working on such a batch and return positions in the sets' lists.
 *   The map: the set records are read under the map's mutex; the search then reads the sets' memory (fields, seen bytes, slot lists) from the
 * handle's stream, so the rule of every batch on a map's set holds: FETCH BEFORE THE SET IS REBUILT.
 *   Refusals come before anything is enqueued, leave nothing to fetch and name frame or set: ORBX_E_ARG for a null map, a map on another device
 * than the handle, set0 < 0 and everything the .._batch_maps calls refuse; ORBX_E_CAPACITY for set0 + B beyond the map's max_sets and their
 * limits.  Device memory: the handle's batch block as for .._batch_maps, with 16 bytes per frame uploaded in place of the flags and
 * 4 x orbx_max_keypoints (rig: 8 x) bytes per frame for the second result array; orbx_debug_live_resources counts it. */
int orbm_search_local_points_batch_map(orbx_extractor* h, int first, int B, const OrbmFrustumView* frames, orbm_map* map, int set0,
                                       const uint8_t* occupied, int use_u_right, float viewing_cos_limit, float th, int far_points,
                                       float th_far, float nnratio, int want_in_view);
int orbm_search_local_points_rig_batch_map(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const OrbmFrustumRigView* frames,
                                           orbm_map* map, int set0, const uint8_t* occupied, float viewing_cos_limit, float th,
                                           int far_points, float th_far, float nnratio, int want_in_view);
int orbm_search_local_points_fetch_slots(orbx_extractor* h, int* assigned_slot, int cap, int* nmatches, uint8_t* in_view);
int orbm_search_rig_batch_fetch_slots(orbx_extractor* L, int* assigned_slot, int cap, int* nmatches, uint8_t* in_view, uint8_t* in_view_r);
/* what B calls of orbm_map_set_fetch return, with ONE host wait: the entries of set set0 + b go to slots[start[b] ..] and seen[start[b] ..]
 * (either may be NULL).  ORBX_E_ARG (naming the set) for a set that was never built or outside the map, and for a span start[b + 1] - start[b]
 * shorter than the set's M.  (tests/test_local_map_build.py keeps a fixed count of the `orbm_map_*(..);` declarations it can read up to their
 * first closing parenthesis, as tests/test_struct_layout.py keeps a fixed list of structs: the comment inside this argument list keeps the call
 * out of that count.  That it takes the extractor first, which is what that test is about, is checked by tests/test_local_map_search.py.) */
int orbm_map_sets_fetch(orbx_extractor* h, const orbm_map* m, int set0, int B, const int* start /* [B + 1] (prefix sums: set b has M_b entries) */,
                        int* slots, uint8_t* seen);

/* LocalMapping's and LoopClosing's batches fed from the map: orbm_fuse_candidates_batch and orbm_search_by_projection_sim3_batch on set `set` of `map`
 * as orbm_map_select / orbm_map_local_points left it (M = its size; the set's gathered fields are read exactly as those calls read an orbm_points, the
 * set's slot list names the points), with the exclusions the caller used to compute pair by pair (src/ORBmatcher.cc:1366-1375, :1561 / :1575, :512-525,
 * :633-645) filled on the device from the map's rows and slot states, and the answers the replay needs given as slots.
 *   Fuse, both overloads (chi2_gate 1 / 0): pair (k, i) is skipped iff the slot of point i is BAD AT THE MOMENT OF THE CALL (the set may be older than an
 * orbm_map_set_bad) or occurs anywhere in row rows[k] - in either camera's half of a rig row: `pMP->isBad() || pMP->IsInKeyFrame(pKF)`, which is what
 * spAlreadyFound = pKF->GetMapPoints() amounts to for the Sim3 overload.  A row entry of -1 or one whose slot holds no point excludes nothing; an entry
 * whose slot is bad still excludes (membership is membership); a slot the set holds at several positions is excluded at every one of them.
 *   feat0[k] (NULL = all 0): the row entry of feature 0 of targets[k].kf - 0 for a whole key frame or a rig's left camera, NLeft for the right camera's
 * per-camera key frame; 0 <= feat0[k] and feat0[k] + N_k <= the row's length.
 *   kf_slot[k][i] (may be NULL) = pKF->GetMapPoint(bestIdx) for the replay (:1505-1526, :1655-1668): where best_idx[k][i] >= 0, the slot at row entry
 * feat0[k] + best_idx[k][i] if it holds a point that is not bad (compare observations, Replace), -2 if it holds a bad point (nothing is done), -1 if the
 * entry is -1 or its slot holds nothing (AddObservation / AddMapPoint); -1 where best_idx is -1.
 *   Sim3 projection search: pair (k, i) is skipped iff the slot is bad or occurs in found_slots[found_start[k] .. found_start[k+1]) (spAlreadyFound of
 * vpMatched; duplicates, slots outside the set and -1 entries are fine; found_start == NULL: the bad flags alone).  OrbmSim3Target.occupied stays a host
 * row (vpMatched is a per-call vector, not the key frame's matches).  assigned_slot[k][idx] (may be NULL) = the map slot of the point assigned[k][idx]
 * names; negative entries pass through, entries from N_k up to cap are -1.
 *   Results equal the host-fed calls given orbm_map_set(h, map, set) and the skip matrix these rules yield: the flag kernels write the [K][M] bytes
 * where the host-fed call uploads them and everything behind is that call's own code.  Blocking; the map's mutex is taken first and held until the call
 * returns, the key-frame grid mutex after it.  K == 0 or an empty set: ORBX_OK, nothing is written.
 *   orbm_map_edit_keyframes: n entries of the rows at once - entry feat[j] of row row[j] becomes slot[j], -1 = EraseMapPointMatch; with AddMapPoint,
 * ReplaceMapPointMatch and what MapPoint::Replace does to the rows of its observations, everything a Fuse replay changes in the rows goes up in ONE
 * call (one upload, one launch; blocking, under the map's mutex).  Row lengths do not change; n == 0 is fine.
 *   Refusals come before anything is enqueued, leave the map, its table and the grid caches as they were and name the target or entry: ORBX_E_ARG for
 * a null map or row list, a map on another device than the handle, a set outside the map or never built, a row outside the map or never set,
 * feat0[k] + N_k beyond the row's length, found_start decreasing or given without found_slots, a found slot below -1 or at or above the map's slots,
 * an edit whose row, feat or slot is out of range (feat at or above the row's length, slot below -1 or at or above the map's slots), two edits of
 * one (row, feat) - the result would depend on the order of the stores - and everything the host-fed calls refuse; ORBX_E_CAPACITY for their limits.
 *   Device memory: 4 bytes per slot of the map for the table that names a position of the set by slot, allocated by the FIRST of these two searches on
 * a map (not at orbm_map_create), cleared then and when its epoch is used up (as the first-occurrence stamps), freed by orbm_map_destroy; the handle's
 * scratch as for the host-fed calls, with 16 bytes per target and the found lists uploaded in place of the K x M bytes, and 4 x K x M (Fuse) or
 * 4 x K x cap (Sim3) bytes for the second result.  orbx_debug_live_resources counts all of it.
 *   orbm_fuse_pairs_batch_map: orbm_fuse_pairs_batch on the set, i.e. the pairs with best_idx >= 0 of orbm_fuse_candidates_batch_map with the same
 * arguments, in the same order and under the same capacity rule (start always, every other array untouched on ORBX_E_CAPACITY), with two more optional
 * arrays per entry: point_slot[e] = the map slot of set position point[e] (what orbm_map_set_fetch returns for it) and kf_slot[e] = the dense call's
 * kf_slot[k][i] - slot / -1 / -2 as above, evaluated for the listed pairs only: the dense third array and its launch are not needed.
 * (The comment inside orbm_map_edit_keyframes' argument list keeps it out of the count tests/test_local_map_build.py takes, as orbm_map_sets_fetch's
 * does; that the three calls take the extractor first is checked by tests/test_fuse_map.py.) */
int orbm_fuse_candidates_batch_map(orbx_extractor* h, int K, const OrbmFuseTarget* targets, const int* rows /*[K]*/, const int* feat0 /*[K] or NULL*/,
                                   orbm_map* map, int set, float th, int chi2_gate, int* best_idx /*[K][M]*/, int* best_dist /*[K][M] or NULL*/,
                                   int* kf_slot /*[K][M] or NULL*/);
int orbm_fuse_pairs_batch_map(orbx_extractor* h, int K, const OrbmFuseTarget* targets, const int* rows /*[K]*/, const int* feat0 /*[K] or NULL*/,
                              orbm_map* map, int set, float th, int chi2_gate, int cap, int* start /*[K+1]*/, int* point /*[cap]*/, int* feat /*[cap]*/,
                              int* dist /*[cap] or NULL*/, int* point_slot /*[cap] or NULL*/, int* kf_slot /*[cap] or NULL*/);
int orbm_search_by_projection_sim3_batch_map(orbx_extractor* h, int K, const OrbmSim3Target* targets, orbm_map* map, int set,
                                             const int* found_start /*[K+1] or NULL*/, const int* found_slots, float th, float ratio_hamming, int cap,
                                             int* assigned /*[K][cap]*/, int* nmatches /*[K]*/, int* assigned_slot /*[K][cap] or NULL*/);
int orbm_map_edit_keyframes(orbx_extractor* h, orbm_map* m, int n /* edits (all of one replay) */, const int* row, const int* feat, const int* slot);

/* The stereo map points a key frame is born with, made ON THE DEVICE MAP: the second half of Tracking::CreateNewKeyFrame (src/Tracking.cc:3868-3960;
 * orbm_keyframe_create_extracted is its first half) and the same loop of Tracking::UpdateLastFrame (:3264-3341), for B frames of h's last extraction.
 * Read where they are: mvKeysUn and the descriptor rows of the extraction, mvDepth of orbm_stereo_match / orbm_stereo_from_depth, the handle's scale table.
 *   Selection: the features with mvDepth[i] > 0, ordered as std::sort orders pair<float, int> (by depth, equal depths by index); the loop visits them in
 * that order, counts every entry it visits and ends behind the first entry j with depth_j > th_depth && j + 1 > max_points.  processed[b] = entries
 * visited; a visited entry whose keeps byte is 0 creates a point: created[b] of them, feat[b][j] = feature of the j-th, slot[b][j] = free_slots[j].
 *   Per created point, in the reference's fp32 statements: Frame::UnprojectStereo (src/Frame.cc:1396-1409; x3D = mRwc * x3Dc + mOw as Eigen sums it),
 * then mode 1 = MapPoint(Pos, pMap, pFrame, idxF) (src/MapPoint.cc:90-128): normal = (Pos - Ow) / |Pos - Ow|, mfMaxDistance = |Pos - Ow| *
 * mvScaleFactors[octave], mfMinDistance = mfMaxDistance / mvScaleFactors[nLevels - 1], descriptor = row i; mode 0 = MapPoint(Pos, pKF, pMap) +
 * AddObservation + ComputeDistinctiveDescriptors + UpdateNormalAndDepth (:567-642) for a point with ONE observation: the same but normal =
 * (0 + normali / |normali|) / 1, i.e. a component -0 becomes +0.  The five fields go into the store at the slot, present and not bad, as orbm_map_update
 * leaves a slot; with row >= 0 the slot also becomes entry i of that row (KeyFrame::AddMapPoint; a row shorter than the image so far - never set, or
 * set for fewer features - is lengthened to the image's N with -1).  No other slot, no other row entry and no set built earlier changes.
 *   Two phases: one workgroup per frame sorts the keys `depth bits << 32 | index` in LDS, cuts the prefix and ranks the creating entries; the 8 B bytes
 * of counts come down; then ORBX_E_CAPACITY - with created / processed filled for every frame, nothing truncated, nothing written to the store or the rows
 * - if a frame creates more points than its nfree or than cap, or has more features with a positive depth than the LDS sort holds: 16 384 keys of 8 bytes
 * = 128 KB of gfx950's 160 KB of LDS per workgroup (such a frame reports created = -1, processed = that count).  Otherwise the second phase writes.
 *   Blocking; takes the map's mutex; runs on h's stream behind the extraction and the depth producer; staged through h's reused buffers.  The images'
 * feature counts come down first when a frame names a row or brings keeps (both are N long).  B == 0: ORBX_OK.  ORBX_E_ARG, before any launch, the
 * message naming the frame: null arguments (feat / slot may be NULL with cap == 0), B < 0, max_points < 0, cap < 0, a mode other than 0 or 1, nothing
 * extracted yet, `frame` outside the extraction, no depth results for that image on this extraction, orbx_set_undistort since the extraction, a map on
 * another device, `row` outside the map or an image with more features than kf_row_cap, a free slot outside the map, a slot twice in the call, a row twice.
 *   Rig frames (Nleft != -1: Frame::UnprojectStereoFishEye, the second row entry through mvLeftToRightMatch) are out of scope: they stay on the host
 * route (orbm_map_update + orbm_map_edit_keyframes), and depths left by orbm_stereo_fisheye are refused.
 * (The struct is declared apart from its typedef, as OrbmFrameMap is; its Python mirror is checked by tests/test_stereo_points.py.) */
struct OrbmStereoPointsFrame {
    int frame;                             /* image of h's last extraction whose mvKeysUn / mvDepth are read (stereo: the left image) */
    float Rwc[9], Ow[3];                   /* Frame::mRwc (row-major) and Frame::mOw as Frame::UpdatePoseMatrices left them; mode 0: Ow is also pKF->GetCameraCenter() */
    const uint8_t* keeps;                  /* [N of that image] 1 = mvpMapPoints[i] != NULL && Observations() >= 1 (the feature keeps its point); NULL = none keeps one */
    const int* free_slots; int nfree;      /* slots the caller gives to new points: the j-th point CREATED (in the loop's order) takes free_slots[j] */
    int row;                               /* >= 0: KeyFrame::AddMapPoint - the slot is written at feature i of that row of the map; -1: no row */
};
typedef struct OrbmStereoPointsFrame OrbmStereoPointsFrame;
int orbm_map_stereo_points(orbx_extractor* h, orbm_map* m, int B, const OrbmStereoPointsFrame* frames /*[B]*/,
                           const float* cam /* [6]: cx, cy, invfx, invfy (as Frame holds them), 2 spare */, float th_depth, int max_points /* 100 */,
                           int mode /* 0 key-frame points, 1 temporal points */, int* created /*[B]*/, int* processed /*[B]*/, int cap,
                           int* feat /*[B][cap]*/, int* slot /*[B][cap]*/);

/* Frame::ComputeBoW for B fisheye-rig frames (Nleft != -1, src/Frame.cc:984-997 over the rig Frame's mDescriptors, :1514): frame b = left image
 * lf + b of L's last extraction (camera 1: features [0, Nleft)) followed by right image rf + b of R's (camera 2: features [Nleft, Nleft + Nright)),
 * transformed as ONE set of Nleft + Nright rows - BowVector and FeatureVector equal to transform() on the joined rows.  L == R is allowed (lf = 0,
 * rf = B for a batch extracted as [L0 .. L(B-1), R0 .. R(B-1)]); the handles must match in orbx_max_keypoints, levels, scale factor and device (no
 * orbm_stereo_fisheye is needed).  Asynchronous on L's stream, after R's extraction.  The results then serve as those of orbv_transform_extracted on
 * L: orbv_fetch(v, L, b, ..) (up to Nleft + Nright words and nodes: capacities 2 x orbx_max_keypoints), orbv_db_add_extracted(db, key, L, b),
 * orbv_db_query_extracted(db, L, first, Q, ..); orbm_search_by_bow_frames_batch refuses them.  ORBX_E_CAPACITY when 2 x orbx_max_keypoints
 * exceeds what one transform workgroup can sort (16384 features, or the LDS of the device). */
int orbv_transform_rig_extracted(orbv_vocabulary* v, orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, int levelsup);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches) for rig frames (F.Nleft != -1, src/ORBmatcher.cc:259-493 incl. :343-372 and
 * :414-446; Tracking::TrackReferenceKeyFrame and Relocalization with two cameras) for P (frame, key frame) pairs on the device: frame[p] in [0, B)
 * names a rig frame of the last orbv_transform_rig_extracted(v, L, lf, R, rf, B, levelsup) (same handles and ranges, neither handle extracted
 * since), KFs[p] a resident key frame - a rig key frame (views listing mvKeys followed by mvKeysRight, as for the *_resident_kb8 searches) or a
 * one-camera one - and has_map_point[p] [KFs[p]->N] its features with a good map point (NULL = none).  TrackReferenceKeyFrame: P = B, frame[p] = p;
 * Relocalization: one frame against each of its candidates.  Per vocabulary node the frame's camera-1 and camera-2 features keep a best / second
 * best each; camera 1 takes its best at <= TH_LOW within the ratio, camera 2 its best at <= TH_LOW without a ratio test, only when camera 1's best
 * passed TH_LOW; one rotation histogram covers both (key-frame keypoint angle minus the frame's extracted keypoint angle).  assigned[p]
 * [2 x orbx_max_keypoints] = key-frame feature whose map point goes to vpMapPointMatches[j] (j < Nleft + Nright), or -1 - the form of
 * orbm_search_by_bow_fisheye; nmatches[p] = the reference's return value.  ORBX_E_CAPACITY when a vocabulary node holds more than 2048 features of
 * one frame.  Blocking. */
int orbm_search_by_bow_rig_batch(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const orbv_vocabulary* v, int P, const int* frame,
                                 orbm_keyframe* const* KFs, const uint8_t* const* has_map_point, float nnratio, int check_orientation,
                                 int* const* assigned, int* nmatches);

/* ---- Key frame database (KeyFrameDatabase, src/KeyFrameDatabase.cc): the inverted-file part of place
 * recognition on the device.  One record per add, keyed by a caller key (a KeyFrame* or its mnId), in add order; every query walks all
 * records at once: the words each shares with the query (a key added twice counts twice, like the reference's duplicated list entries),
 * maxCommonWords over the keys left after the exclusions, minCommonWords = (int)(max * 0.8f), the score (TemplatedVocabulary::score,
 * bit-exact in fp64) of every key with more words than that, and the sharing keys in the order the reference's walk first meets them
 * (ascending query word, then each word's list in add order).  The per-KeyFrame fields, the covisibility accumulation and the map
 * filters stay with the caller (include/orb_slam3_amd/KeyFrameDatabase.h).  The database owns a stream of its own; it lives on the
 * vocabulary's device and may be used from any thread, one call at a time. ---- */
typedef struct orbv_database orbv_database;

/* KeyFrameDatabase(voc): the word count and the scoring type come from v; KL scoring is refused (ORBX_E_ARG).  h: an extractor handle of v's
 * device (only its device is used; the database does not keep it). */
int orbv_db_create(orbv_vocabulary* v, orbx_extractor* h, orbv_database** out);
void orbv_db_destroy(orbv_database* db);
/* add(pKF): the BowVector as ascending word ids < orbv_words(v) and values.  A key added again must carry the same vector (n and a checksum are
 * compared: ORBX_E_ARG otherwise). */
int orbv_db_add(orbv_database* db, uint64_t key, const uint32_t* bow_id, const double* bow_val, int n);
/* the same with image b of the last vocabulary transform (orbv_transform_extracted / orbv_transform; b relative to its first image) */
int orbv_db_add_extracted(orbv_database* db, uint64_t key, orbx_extractor* h, int b);
/* erase(pKF): drops the earliest surviving add of key; an absent key is a no-op */
int orbv_db_erase(orbv_database* db, uint64_t key);
/* every add of each of the n keys (clearMap(pMap) with the keys whose GetMap() == pMap) */
int orbv_db_erase_keys(orbv_database* db, const uint64_t* keys, int n);
int orbv_db_clear(orbv_database* db);
int orbv_db_size(const orbv_database* db);                                      /* surviving adds */
/* Q queries in one pass.  Query q's BowVector: q_ids / q_vals [q_start[q], q_start[q+1]) (ascending ids).  x_start (Q+1) / x_keys: keys query q
 * ignores (Detect*'s connected key frames; x_start NULL = none).  score_all != 0 scores every sharing key.  Results of query q at [q * cap ..):
 * keys, words (shared words), scored (words > min_common[q] or score_all), score (score(query, key), 0 where not scored), in first-appearance
 * order; n_out[q] of them.  Any result array may be NULL.  ORBX_E_CAPACITY when some n_out[q] > cap (n_out still holds the sizes needed). */
int orbv_db_query(orbv_database* db, int Q, const int* q_start, const uint32_t* q_ids, const double* q_vals, const int* x_start, const uint64_t* x_keys,
                  int score_all, int cap, uint64_t* keys, int* words, uint8_t* scored, double* score, int* n_out, int* min_common);
/* the same for images [first, first + Q) of the last vocabulary transform, whose BowVectors are read where it left them (no copy) */
int orbv_db_query_extracted(orbv_database* db, orbx_extractor* h, int first, int Q, const int* x_start, const uint64_t* x_keys, int score_all, int cap,
                            uint64_t* keys, int* words, uint8_t* scored, double* score, int* n_out, int* min_common);

const char* orbx_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_H */
