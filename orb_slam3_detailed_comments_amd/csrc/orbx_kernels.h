// orbx_kernels.h — prototypes of the __global__ kernels (defined in k_*.hip) for the host launcher.
#pragma once
#include "orbx_types.h"
#include "undistort_model.h"

namespace orbx {

__global__ void k_import(const LevelInfo* __restrict__ lv, const uint8_t* __restrict__ images, int stride,
                         size_t image_stride, uint8_t* __restrict__ pyr, size_t pyr_stride);
__global__ void k_resize(const LevelInfo* __restrict__ lv, int level, const ResizeTap* __restrict__ xtab,
                         const ResizeTap* __restrict__ ytab, uint8_t* __restrict__ pyr, size_t pyr_stride,
                         int lds_pitch, int lds_rows);
// strip_rows (<= 64): output rows per wave; a block covers 256 columns x 4 strips
__global__ void k_resize_rows(const LevelInfo* __restrict__ lv, int level, const ResizeTap* __restrict__ xtab,
                              const ResizeTap* __restrict__ ytab, uint8_t* __restrict__ pyr, size_t pyr_stride, int strip_rows);
#ifndef ORBX_PYR_THREADS
#define ORBX_PYR_THREADS 512
#endif
#ifndef ORBX_PYR_TILE
#define ORBX_PYR_TILE 16
#endif
constexpr int kPyrTile = ORBX_PYR_TILE;        // k_pyramid_fused: a workgroup's tile of the top pyramid level
constexpr int kPyrThreads = ORBX_PYR_THREADS;  // ... and its threads (the tile is a latency problem: many waves per tile)
__global__ void k_pyramid_fused(const LevelInfo* __restrict__ lv, int nlevels, const ResizeTap* __restrict__ xtab, const ResizeTap* __restrict__ ytab,
                                const PyrSpan* __restrict__ xspan, const PyrSpan* __restrict__ yspan, int ntx, uint8_t* __restrict__ pyr, size_t pyr_stride,
                                int buf_a_bytes, int buf_b_bytes, PyrTapOffsets toff);
#ifndef ORBX_FAST_XCD_RUN
#define ORBX_FAST_XCD_RUN 4
#endif
constexpr int kFastXcdRun = ORBX_FAST_XCD_RUN;   // neighbouring FAST cells kept on one XCD (k_fast_cells)
constexpr int kFastThreadsDecl = 64;   // must equal kFastThreads in k_fast.hip
constexpr int kFastPitch = 48;         // LDS pitch of the FAST window tile for cells whose dword-aligned window fits in it (cells up to 39 px wide)
__global__ void k_fast_cells(const LevelInfo* __restrict__ lv, const CellInfo* __restrict__ cells, int ncells,
                             const uint8_t* __restrict__ pyr, size_t pyr_stride, int iniTh, int minTh,
                             uint32_t* __restrict__ slots, size_t slots_stride, int* __restrict__ cell_count,
                             int tile_bytes, int list_bytes, int* __restrict__ status);
// bordered copy of every level (ORB-SLAM3's mvImagePyramid layout, BORDER_REFLECT_101): grid (fl.band[nlevels], B), block 256; a workgroup writes
// kFrameRows framed rows of one level, a lane 16 bytes per store
constexpr int kFrameRows = 8;
__global__ void k_frame_pyramid(const LevelInfo* __restrict__ lv, int nlevels, const uint8_t* __restrict__ pyr, size_t pyr_stride,
                                uint8_t* __restrict__ out, size_t out_stride, FrameLayout fl);
constexpr int kResizeRows = 8;         // output rows per k_resize tile (256 columns wide)
// Output rows per k_blur wave (a block covers 256 columns x 4 strips of that many rows).  A strip reads 6 halo rows on top of its own: large batches
// run strips of 32 rows (the horizontal pass of 38 input rows per 32 outputs instead of 22 per 16: +1.0 % on the headline, profiles/r06/ab_experiments.txt),
// small batches - where the number of waves in flight is what counts, and the blur shares its launch with the FAST cells - strips of 16.
#ifndef ORBX_BLUR_ROWS
#define ORBX_BLUR_ROWS 16
#endif
#ifndef ORBX_BLUR_ROWS_LARGE
#define ORBX_BLUR_ROWS_LARGE 32
#endif
constexpr int kBlurRows = ORBX_BLUR_ROWS, kBlurRowsLarge = ORBX_BLUR_ROWS_LARGE;
constexpr int kSimdSelftestOps = 22;
__global__ void k_simd_selftest(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, const uint32_t* __restrict__ c, int n, uint32_t* __restrict__ out);
constexpr int kModelSelftestOps = 8, kModelSelftestMax = 1 << 26;      // orbx_debug_model_eval (k_describe.hip): ops 0 .. 7, elements per call
__global__ void k_model_selftest(int op, uint32_t start_bits, const float* __restrict__ a, const float* __restrict__ b, int n, float* __restrict__ out);
__global__ void k_blur(const LevelInfo* __restrict__ lv, int nlevels, const uint8_t* __restrict__ pyr,
                       uint8_t* __restrict__ blur, size_t pyr_stride, BlurTaps taps, BlurTiles tiles);
__global__ void k_blur_large(const LevelInfo* __restrict__ lv, int nlevels, const uint8_t* __restrict__ pyr,
                             uint8_t* __restrict__ blur, size_t pyr_stride, BlurTaps taps, BlurTiles tiles);     // strips of kBlurRowsLarge rows
constexpr int kQuadtreeThreads = 1024; // workgroup size of k_quadtree; a level uses its first LevelInfo::qt_threads threads
// small batches: the blur strips and the FAST cells of an image in one launch (k_fast.hip)
__global__ void k_fast_cells_blur(const LevelInfo* __restrict__ lv, const CellInfo* __restrict__ cells, int ncells,
                                  const uint8_t* __restrict__ pyr, size_t pyr_stride, int iniTh, int minTh,
                                  uint32_t* __restrict__ slots, size_t slots_stride, int* __restrict__ cell_count,
                                  int tile_bytes, int list_bytes, int* __restrict__ status,
                                  int nlevels, uint8_t* __restrict__ blur, BlurTaps taps, BlurTiles tiles, int blur_waves);
__global__ void k_quadtree(const LevelInfo* __restrict__ lv, const CellInfo* __restrict__ cells, int ncells,
                           const int* __restrict__ cell_count, const uint32_t* __restrict__ slots, size_t slots_stride,
                           uint32_t* __restrict__ candA, uint32_t* __restrict__ candB, size_t cand_stride,
                           uint32_t* __restrict__ lvl_keys, int kp_total_cap, int* __restrict__ lvl_count,
                           int nlevels, int node_cap, int nb_cap, int lut_x, int lut_y, int* __restrict__ status, long long* __restrict__ qt_prof,
                           int wide, int counter_bytes, int level0, int* __restrict__ qt_sorted, int eager);
// levels whose node lists exceed the LDS (the 5 x nFeatures extractor of the monocular initialisation): node arrays in a global pool
__global__ void k_quadtree_spill(const LevelInfo* __restrict__ lv, const CellInfo* __restrict__ cells, int ncells,
                           const int* __restrict__ cell_count, const uint32_t* __restrict__ slots, size_t slots_stride,
                           uint32_t* __restrict__ candA, uint32_t* __restrict__ candB, size_t cand_stride,
                           uint32_t* __restrict__ lvl_keys, int kp_total_cap, int* __restrict__ lvl_count,
                           int nlevels, int node_cap, int nb_cap, int lut_x, int lut_y, int* __restrict__ status, long long* __restrict__ qt_prof,
                           int wide, int counter_bytes, unsigned char* __restrict__ pool, size_t pool_stride, int* __restrict__ qt_sorted, int eager);
constexpr int kQuadtreeLdsNodes = 4000;     // the LDS form packs positions of its sort ranges in 12 bits: trees with more nodes take the pool form whatever the LDS
// self-test of the quadtree's workgroup primitives (orbx_debug_quadtree_selftest; k_quadtree.hip): one workgroup of 256 or 1024 threads.
// The sort's arrays: two range lists of quadtree_selftest_seg_cap(n) entries (4 bytes in the LDS form, 8 in the pool form), two arrays of n keys, n flag bytes.
ORBX_HD constexpr int quadtree_selftest_seg_cap(int n) { return (n / 8 + 8 + 1) & ~1; }
ORBX_HD constexpr size_t quadtree_selftest_sort_bytes(int n, bool spill) { return (size_t)quadtree_selftest_seg_cap(n) * 2 * (spill ? 8 : 4) + (size_t)n * 17 + 16; }
__global__ void k_quadtree_selftest(int op, int spill, const void* __restrict__ in, void* __restrict__ out, unsigned char* __restrict__ pool,
                                    int n, int s, int total, int mx, int my);
__global__ void k_layout(const LevelInfo* __restrict__ lv, int nlevels, const uint32_t* __restrict__ lvl_keys,
                         int kp_total_cap, const int* __restrict__ lvl_count, int lap0, int lap1,
                         int* __restrict__ final_idx, int* __restrict__ n_out, int* __restrict__ mono_out,
                         int nb, int* __restrict__ row_start, int* __restrict__ row_pos);
#ifndef ORBX_STEREO_ROW_SHIFT
#define ORBX_STEREO_ROW_SHIFT 3
#endif
constexpr int kStereoRowShift = ORBX_STEREO_ROW_SHIFT;   // k_layout / k_stereo_match: right keypoints are bucketed by (first row of their band) >> shift
// search record of a keypoint (k_orient_brief -> k_stereo_match), stored at the keypoint's place in the bucket order: {first row, last row of its
// candidate band, x bits, octave | output index << kAuxIndexShift} (octave < kMaxLevels, index < 65535)
constexpr int kAuxIndexShift = 8;
constexpr int kKpPerWaveDecl = 8;     // must equal kKpPerWave in k_describe.hip
constexpr int kKpPerWaveSmallDecl = 2; // keypoints per wave of k_orient_brief_small
__global__ void k_orient_brief(const LevelInfo* __restrict__ lv, int nlevels, const uint8_t* __restrict__ pyr,
                               const uint8_t* __restrict__ blur, size_t pyr_stride,
                               const uint32_t* __restrict__ lvl_keys, int kp_total_cap,
                               const int* __restrict__ lvl_count, const int* __restrict__ final_idx, const int* __restrict__ row_pos, UmaxTab umax,
                               KeyPointRec* __restrict__ out_kps, unsigned long long* __restrict__ out_desc, int4* __restrict__ out_aux,
                               int B, int groups_per_image);
__global__ void k_orient_brief_small(const LevelInfo* __restrict__ lv, int nlevels, const uint8_t* __restrict__ pyr,
                               const uint8_t* __restrict__ blur, size_t pyr_stride,
                               const uint32_t* __restrict__ lvl_keys, int kp_total_cap,
                               const int* __restrict__ lvl_count, const int* __restrict__ final_idx, const int* __restrict__ row_pos, UmaxTab umax,
                               KeyPointRec* __restrict__ out_kps, unsigned long long* __restrict__ out_desc, int4* __restrict__ out_aux,
                               int B, int groups_per_image);
__global__ void k_undistort(const KeyPointRec* __restrict__ kps, const int* __restrict__ n_per_frame, int cap, UndistortParams U, KeyPointRec* __restrict__ kps_un);
__global__ void k_hamming_matrix(const unsigned long long* __restrict__ A, int na,
                                 const unsigned long long* __restrict__ Bm, int nb, int* __restrict__ out);
__global__ void k_stereo_match(const LevelInfo* __restrict__ lv, const KeyPointRec* __restrict__ kpsL,
                               const unsigned long long* __restrict__ descL, const int* __restrict__ nL,
                               const unsigned long long* __restrict__ descR,
                               const int4* __restrict__ auxR, const int* __restrict__ nR, const int* __restrict__ bucket_start,
                               int nb, int lookback, int cap, const uint8_t* __restrict__ pyrL,
                               const uint8_t* __restrict__ pyrR, size_t pyr_stride, StereoParams P,
                               float* __restrict__ uRight, float* __restrict__ depth, int* __restrict__ sad);
__global__ void k_stereo_median(const int* __restrict__ nL, int cap, float* __restrict__ uRight,
                                float* __restrict__ depth, const int* __restrict__ sad, int* __restrict__ n_matches);
__global__ void k_kb8_stereo(const KeyPointRec* __restrict__ kpsL, const int* __restrict__ monoL, const int* __restrict__ nL,
                             const KeyPointRec* __restrict__ kpsR, const int* __restrict__ monoR, int cap, const int* __restrict__ idx0,
                             const uint8_t* __restrict__ ratio_ok, KB8StereoParams P, int* __restrict__ l2r, int* __restrict__ r2l,
                             float* __restrict__ depth, float* __restrict__ p3d, int* __restrict__ nmatches);
__global__ void k_knn2_mfma(const unsigned long long* __restrict__ descQ, const int* __restrict__ qoff, const int* __restrict__ nq,
                            const unsigned long long* __restrict__ descT, const int* __restrict__ toff, const int* __restrict__ nt, int cap,
                            int* __restrict__ idx0, int* __restrict__ dist0, int* __restrict__ idx1, int* __restrict__ dist1, uint8_t* __restrict__ ratio_ok);
__global__ void k_knn2(const unsigned long long* __restrict__ descQ, const int* __restrict__ qoff, const int* __restrict__ nq,
                       const unsigned long long* __restrict__ descT, const int* __restrict__ toff, const int* __restrict__ nt,
                       int cap, int* __restrict__ idx0, int* __restrict__ dist0, int* __restrict__ idx1,
                       int* __restrict__ dist1, uint8_t* __restrict__ ratio_ok);

constexpr int kGridThreads = 1024;     // workgroup size of k_grid_build (3 grid cells per thread)
constexpr int kGridCellStride = 64 * 48 + 2;   // ints per frame of the batched cell_start arrays
__global__ void k_grid_build(const KeyPointRec* __restrict__ kps, int N, GridParams g, int* __restrict__ cell_of,
                             int* __restrict__ cell_start, int* __restrict__ cell_items, const int* __restrict__ n_per_frame, int frame_stride);
__global__ void k_grid_build_kfs(const GridBuildRec* __restrict__ recs);
__global__ void k_fuse_candidates(const FuseTargetRec* __restrict__ T, int M, const float* __restrict__ pos, const float* __restrict__ normal, const float* __restrict__ min_d,
                                  const float* __restrict__ max_d, const unsigned long long* __restrict__ qdesc, const uint8_t* __restrict__ skip, float th, int chi2_gate,
                                  int th_low, int debug_flags, int* __restrict__ best_idx, int* __restrict__ best_dist);
__global__ void k_sim3_candidates(const Sim3TargetRec* __restrict__ T, int M, const float* __restrict__ pos, const float* __restrict__ normal, const float* __restrict__ min_d,
                                  const float* __restrict__ max_d, const unsigned long long* __restrict__ qdesc, const uint8_t* __restrict__ occupied,
                                  const uint8_t* __restrict__ skip, float th, float max_dist, int debug_flags, int* __restrict__ choice);
__global__ void k_sim3_accept(const Sim3TargetRec* __restrict__ T, int M, const float* __restrict__ pos, const float* __restrict__ normal, const float* __restrict__ min_d,
                              const float* __restrict__ max_d, const unsigned long long* __restrict__ qdesc, const uint8_t* __restrict__ occupied, float th, float max_dist,
                              int debug_flags, int cap, const int* __restrict__ choice, int* __restrict__ assigned, int* __restrict__ nmatches);
constexpr int kAreaWaves = 16;         // queries (waves) per k_area_search workgroup
__global__ void k_area_search(const AreaQuery* __restrict__ queries, const unsigned long long* __restrict__ qdesc, int Q,
                              const KeyPointRec* __restrict__ kps, const float* __restrict__ u_right,
                              const unsigned long long* __restrict__ fdesc, GridParams g, const int* __restrict__ cell_start,
                              const int* __restrict__ cell_items, int gate_right, int* __restrict__ pool_counter, int pool_cap,
                              int* __restrict__ q_start, int* __restrict__ q_count, int2* __restrict__ entries);
__global__ void k_frustum(FrustumParams F, int M, const float* __restrict__ pos, const float* __restrict__ normal, const float* __restrict__ min_dist,
                          const float* __restrict__ max_dist, const uint8_t* __restrict__ is_bad, uint8_t* __restrict__ in_view, float* __restrict__ track,
                          int* __restrict__ scale_level, AreaQuery* __restrict__ queries, int* __restrict__ zero4);
__global__ void k_frustum_batch(const FrustumParams* __restrict__ Fb, const FrameMapRec* __restrict__ maps, const uint8_t* __restrict__ is_bad, uint8_t* __restrict__ in_view,
                                float* __restrict__ track, int* __restrict__ scale_level, AreaQuery* __restrict__ queries, int* __restrict__ zero4);
__global__ void k_project_points(ProjectParams P, int M, const float* __restrict__ pos, const float* __restrict__ normal, const float* __restrict__ min_inv,
                                 const float* __restrict__ max_inv, const uint8_t* __restrict__ skip, uint8_t* __restrict__ valid, float* __restrict__ out, int debug_flags);
__global__ void k_area_search_threads(const AreaQuery* __restrict__ queries, const FrameMapRec* __restrict__ maps, const KeyPointRec* __restrict__ kps,
                                      const float* __restrict__ u_right, const unsigned long long* __restrict__ fdesc, GridParams g,
                                      const int* __restrict__ cell_start, const int* __restrict__ cell_items, int gate_right, int* __restrict__ pool_counter,
                                      int pool_cap, int* __restrict__ q_start, int* __restrict__ q_count, int2* __restrict__ entries, int frame_stride);
__global__ void k_lastframe_queries(const FrustumParams* __restrict__ Fb, int capL, const int* __restrict__ n_last, const float* __restrict__ pos,
                                    const uint8_t* __restrict__ valid, const int* __restrict__ octave, AreaQuery* __restrict__ queries, int* __restrict__ zero4);
__global__ void k_keyframe_queries(const FrustumParams* __restrict__ Fb, int capL, const int* __restrict__ n_kf, const float* __restrict__ pos,
                                   const uint8_t* __restrict__ valid, const float* __restrict__ min_dist, const float* __restrict__ max_dist,
                                   AreaQuery* __restrict__ queries, int* __restrict__ zero4);
__global__ void k_lastframe_accept(const FrameMapRec* __restrict__ maps, int cap, const int* __restrict__ n_per_frame, const int* __restrict__ q_start,
                                   const int* __restrict__ q_count, const int2* __restrict__ entries, const uint8_t* __restrict__ occupied0,
                                   const uint8_t* __restrict__ has_obs, int th_high, int* __restrict__ assigned, int* __restrict__ nmatches,
                                   const float* __restrict__ last_angle, const KeyPointRec* __restrict__ cur_kps, int check_ori);
__global__ void k_local_accept(const FrameMapRec* __restrict__ maps, int cap, const int* __restrict__ n_per_frame, const int* __restrict__ q_start,
                               const int* __restrict__ q_count, const int2* __restrict__ entries, const uint8_t* __restrict__ occupied0,
                               const uint8_t* __restrict__ has_obs, float nnratio, int th_high, int* __restrict__ assigned, int* __restrict__ nmatches);
__global__ void k_frustum_rig(const FrustumParams* __restrict__ Fb, const FrameMapRec* __restrict__ maps, const uint8_t* __restrict__ is_bad, uint8_t* in_view1,
                              uint8_t* in_view2, float* track1, float* track2, int* level1, int* level2, AreaQuery* __restrict__ q1, AreaQuery* __restrict__ q2,
                              int* __restrict__ zero4);
__global__ void k_lastframe_queries_rig(const FrustumParams* __restrict__ Fb, int capL, const int* __restrict__ n_last, const float* __restrict__ pos,
                                        const uint8_t* __restrict__ valid, const int* __restrict__ octave, RigRelPose trl, AreaQuery* q1,
                                        AreaQuery* __restrict__ q2, int* __restrict__ zero4);
__global__ void k_rig_local_accept(const FrameMapRec* __restrict__ maps, int cap, const int* __restrict__ n1, const int* __restrict__ n2, const int* __restrict__ qs1,
                                   const int* __restrict__ qc1, const int* __restrict__ qs2, const int* __restrict__ qc2, const int2* __restrict__ entries,
                                   const uint8_t* __restrict__ occupied0, const uint8_t* __restrict__ has_obs, const int* __restrict__ l2r,
                                   const int* __restrict__ r2l, float nnratio, int th_high, int* __restrict__ assigned, int* __restrict__ nmatches);
__global__ void k_rig_lastframe_accept(const FrameMapRec* __restrict__ maps, int cap, const int* __restrict__ n1, const int* __restrict__ n2, const int* __restrict__ qs1,
                                       const int* __restrict__ qc1, const int* __restrict__ qs2, const int* __restrict__ qc2, const int2* __restrict__ entries,
                                       const uint8_t* __restrict__ occupied0, const uint8_t* __restrict__ has_obs, int th_high, int* __restrict__ assigned,
                                       int* __restrict__ nmatches, const float* __restrict__ last_angle, const KeyPointRec* __restrict__ kps1,
                                       const KeyPointRec* __restrict__ kps2, int check_ori);
__global__ void k_stereo_from_depth(const KeyPointRec* __restrict__ kps, const KeyPointRec* __restrict__ kps_un, const int* __restrict__ n_per_frame, int cap,
                                    const float* __restrict__ depth, int stride, size_t image_stride, int w, int h, float mbf, float* __restrict__ u_right,
                                    float* __restrict__ depth_out, int* __restrict__ n_valid);
__global__ void k_bow_search(const BowItem* __restrict__ items, int nitems, const KeyPointRec* __restrict__ kps1,
                             const unsigned long long* __restrict__ desc1, const float* __restrict__ ur1,
                             const KeyPointRec* __restrict__ kps2, const unsigned long long* __restrict__ desc2,
                             const float* __restrict__ ur2, const uint8_t* __restrict__ has_mp2, const int* __restrict__ feat2,
                             const BowParams* __restrict__ Ps, int* __restrict__ best2);
__global__ void k_bow_search_kb8(const BowItem* __restrict__ items, int nitems, const KeyPointRec* __restrict__ kps1,
                             const unsigned long long* __restrict__ desc1, const float* __restrict__ ur1,
                             const KeyPointRec* __restrict__ kps2, const unsigned long long* __restrict__ desc2,
                             const float* __restrict__ ur2, const uint8_t* __restrict__ has_mp2, const int* __restrict__ feat2,
                             const BowParams* __restrict__ Ps, int* __restrict__ best2);
__global__ void k_sft_resident(ResidentKF k1, const uint8_t* __restrict__ flags, const SftNeighbour* __restrict__ nb, int* __restrict__ best);
__global__ void k_keyframe_counts(const KfSnapRec* __restrict__ recs, int n, int* __restrict__ out);
__global__ void k_keyframe_snapshot(const KfSnapRec* __restrict__ recs);
__global__ void k_sft_resident_kb8(ResidentKF k1, const uint8_t* __restrict__ flags, const SftNeighbour* __restrict__ nb, int* __restrict__ best);
__global__ void k_bow_match_resident(const BowPairResident* __restrict__ pairs, const uint8_t* __restrict__ flags, float nnratio, int th_low,
                                     int th_inclusive, int* __restrict__ m12, int N1cap, int* __restrict__ status);
__global__ void k_bow_rotation_prune(const BowPairResident* __restrict__ pairs, int* __restrict__ m12, int N1cap, int check_ori, int* __restrict__ nmatches);
__global__ void k_bow_match_rig(const BowPairRig* __restrict__ pairs, const uint8_t* __restrict__ flags, float nnratio, int th_low,
                                int* __restrict__ assigned, int S, int* __restrict__ status);
__global__ void k_bow_rotation_prune_rig(const BowPairRig* __restrict__ pairs, int* __restrict__ assigned, int S, int check_ori, int* __restrict__ nmatches);
__global__ void k_bow_dists(const BowItem* __restrict__ items, int nitems, const unsigned long long* __restrict__ desc1,
                            const unsigned long long* __restrict__ desc2, const uint8_t* __restrict__ eligible2,
                            const int* __restrict__ feat2, int* __restrict__ out);
// the resident map (orbm_map): field scatter, and Tracking::UpdateLocalPoints as stamp / count / scan / compact / gather
__global__ void k_map_scatter(int n, const int* __restrict__ slots, const unsigned long long* __restrict__ desc, const float* __restrict__ pos,
                              const float* __restrict__ normal, const float* __restrict__ min_d, const float* __restrict__ max_d, const uint8_t* __restrict__ bad,
                              MapStore S);
__global__ void k_map_seen(const int* __restrict__ seen_start, const int* __restrict__ seen_slots, unsigned* __restrict__ seen_stamp, int nslots, unsigned mark);
__global__ void k_map_stamp(const MapSeg* __restrict__ segs, const int* __restrict__ kf_slots, int row_cap, const uint8_t* __restrict__ state,
                            unsigned* __restrict__ stamp, int nslots, unsigned top);
__global__ void k_map_compact(const MapSeg* __restrict__ segs, const int* __restrict__ kf_slots, int row_cap, const uint8_t* __restrict__ state,
                              const unsigned* __restrict__ stamp, int nslots, unsigned top, int* __restrict__ chunk_cnt, const int* __restrict__ chunk_off,
                              const MapSetRec* __restrict__ sets);
__global__ void k_map_scan(const int* __restrict__ frame_chunk0, const int* __restrict__ chunk_cnt, int* __restrict__ chunk_off, int* __restrict__ M_out);
__global__ void k_map_gather(const MapSetRec* __restrict__ sets, MapStore S, const unsigned* __restrict__ seen_stamp, int nslots, unsigned base);
// the rows of a projection batch (LastFrame / KeyFrame points) and the flags of a BoW batch, read from the map by slot
__global__ void k_map_rows_gather(MapStore S, int cap, const int* __restrict__ n, const int* __restrict__ slots, const MapRowRec* __restrict__ rows,
                                  const uint8_t* __restrict__ excluded, uint8_t* __restrict__ valid, float* __restrict__ pos, unsigned long long* __restrict__ desc,
                                  float* __restrict__ min_d, float* __restrict__ max_d, float* __restrict__ angle);
__global__ void k_map_row_flags(const int* __restrict__ kf_slots, int row_cap, const uint8_t* __restrict__ state, const MapRowFlagRec* __restrict__ recs,
                                uint8_t* __restrict__ flags);
// a batched SearchLocalPoints on the map's own sets: the call-time flags from the sets' seen bytes, and `assigned` as map slots
__global__ void k_map_set_flags(const SetFlagRec* __restrict__ recs, uint8_t* __restrict__ bad, uint8_t* __restrict__ obs);
__global__ void k_assigned_slots(const SetFlagRec* __restrict__ recs, const int* __restrict__ assigned, int S, int* __restrict__ out);
// a Fuse / Sim3 projection batch fed from the map: skip[K][M] from the slots' bad flags and the targets' rows or found lists, the replay's GetMapPoint as
// slots, and the replay's row changes as one sparse edit
__global__ void k_map_set_table(int M, int K, const int* __restrict__ slots, const uint8_t* __restrict__ state, unsigned* __restrict__ table, unsigned top,
                                uint8_t* __restrict__ skip);
__global__ void k_map_skip_listed(const MapSkipRec* __restrict__ recs, const int* __restrict__ lists, int M, const unsigned* __restrict__ table, unsigned base,
                                  unsigned top, uint8_t* __restrict__ skip);
__global__ void k_map_skip_dups(int M, int K, const int* __restrict__ slots, const unsigned* __restrict__ table, unsigned top, uint8_t* __restrict__ skip);
__global__ void k_fuse_kf_slots(const MapSkipRec* __restrict__ recs, const int* __restrict__ kf_slots, int M, const uint8_t* __restrict__ state,
                                const int* __restrict__ best_idx, int* __restrict__ kf_slot);
// the matched pairs of a Fuse batch as one list in the replay's order: count per chunk, scan (tiles, then their sums), scatter
__global__ void k_fuse_pairs(int M, const int* __restrict__ best_idx, const int* __restrict__ best_dist, int* __restrict__ chunk_cnt, const int* __restrict__ chunk_off,
                             const int* __restrict__ tile_off, int ntiles, int cap, int* __restrict__ start, const MapSkipRec* __restrict__ recs,
                             const int* __restrict__ kf_slots, const uint8_t* __restrict__ state, const int* __restrict__ set_slots, FusePairOut O);
__global__ void k_fuse_pair_scan_tiles(int n, const int* __restrict__ chunk_cnt, int* __restrict__ chunk_off, int* __restrict__ tile_sum);
__global__ void k_fuse_pair_scan_sums(int ntiles, const int* __restrict__ tile_sum, int* __restrict__ tile_off);
__global__ void k_map_edit_rows(int n, const int* __restrict__ row, const int* __restrict__ feat, const int* __restrict__ slot, int* __restrict__ kf_slots,
                                int row_cap);
// orbm_map_stereo_points: the depth-ordered selection of Tracking::CreateNewKeyFrame / UpdateLastFrame per frame, then the new points into the store and rows
__global__ void k_map_stereo_select(const StereoPointsRec* __restrict__ recs, StereoPointsParams P, const uint8_t* __restrict__ keeps_all, int* __restrict__ feat_all,
                                    int* __restrict__ counts);
__global__ void k_map_stereo_write(const StereoPointsRec* __restrict__ recs, StereoPointsParams P, const int* __restrict__ free_all, const int* __restrict__ feat_all,
                                   const int* __restrict__ counts, MapStore S, int* __restrict__ kf_slots, int row_cap, int* __restrict__ out_feat);

__global__ void k_distinctive(const unsigned long long* __restrict__ desc, const int* __restrict__ start, int P, int* __restrict__ best);
template <bool kLds>        // instantiated for both forms in k_match.hip
__global__ void k_distinctive_resident(const DistinctiveRec* __restrict__ recs, int first, int count,
                                       const unsigned long long* const* __restrict__ kf_desc, const int* __restrict__ obs_kf, const int* __restrict__ obs_feat,
                                       int* __restrict__ best, unsigned long long* __restrict__ best_desc);
__global__ void k_voc_descend(const unsigned long long* __restrict__ fdesc, const int* __restrict__ n_feat, int n_fixed, int cap, int B,
                              const unsigned long long* __restrict__ slot_desc, const VocSlot* __restrict__ slots,
                              const double* __restrict__ slot_weight, int root_children, int nid_level, unsigned* __restrict__ out_word,
                              unsigned* __restrict__ out_node, double* __restrict__ out_weight);
__global__ void k_voc_gather_rig(const unsigned long long* __restrict__ desc_l, const int* __restrict__ n_l, const unsigned long long* __restrict__ desc_r,
                                 const int* __restrict__ n_r, int cap, int B, unsigned long long* __restrict__ out, int* __restrict__ n_out);
__global__ void k_voc_assemble(const unsigned* __restrict__ word, const unsigned* __restrict__ node, const double* __restrict__ weight,
                               const int* __restrict__ n_feat, int n_fixed, int cap, int P, int weighting, int norm,
                               unsigned* __restrict__ bow_id, double* __restrict__ bow_val, int* __restrict__ bow_start,
                               unsigned* __restrict__ fv_node, int* __restrict__ fv_start, unsigned* __restrict__ fv_feat,
                               int* __restrict__ n_out);
__global__ void k_kfdb_count(const unsigned* __restrict__ ids, const long long* __restrict__ rstart, const int* __restrict__ rn,
                             const int* __restrict__ rmult, int R, KfdbQuerySet qs, int* __restrict__ cnt, int* __restrict__ firstpos);
__global__ void k_kfdb_order(int* __restrict__ cnt, const int* __restrict__ firstpos, const unsigned long long* __restrict__ rkey, int R,
                             const int* __restrict__ qn, int qn_step, const int* __restrict__ xstart, const int* __restrict__ xrec, int score_all,
                             int* __restrict__ order, KfdbHit* __restrict__ hits, int* __restrict__ slist, int* __restrict__ head);
__global__ void k_kfdb_score(const unsigned* __restrict__ ids, const double* __restrict__ vals, const long long* __restrict__ rstart,
                             const int* __restrict__ rn, KfdbQuerySet qs, const int* __restrict__ order, const int* __restrict__ slist,
                             const int* __restrict__ head, KfdbHit* __restrict__ hits, int R, int scoring);

__global__ void k_input_remap(const uint8_t* __restrict__ src, int sw, int sh, int sstride, size_t simg, int C, const float* __restrict__ mapx,
                              const float* __restrict__ mapy, int out_w, int out_h, uint8_t* __restrict__ dst, int dst_pitch, size_t dst_stride);
__global__ void k_input_resize(const uint8_t* __restrict__ src, int sw, int sh, int sstride, size_t simg, int C, const ResizeTap* __restrict__ xt,
                               const ResizeTap* __restrict__ yt, int out_w, int out_h, uint8_t* __restrict__ dst, int dst_pitch, size_t dst_stride);
__global__ void k_input_gray(const uint8_t* __restrict__ src, int sstride, size_t simg, int C, int ridx, int ry, int gy, int by, int shift, int w, int h,
                             uint8_t* __restrict__ dst, int dst_pitch, size_t dst_stride);

}  // namespace orbx
