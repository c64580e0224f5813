// orbx_types.h — device-visible tables and packed record formats shared by the kernels and the host.
#pragma once
#include <cstdint>
#include "orbx_platform.h"

namespace orbx {

constexpr int kMaxLevels = 16;
constexpr int kEdge = 19;        // EDGE_THRESHOLD, reference src/ORBextractor.cc:78
constexpr int kBorder = 16;      // minBorderX/Y = EDGE_THRESHOLD-3, :1076-1077
constexpr int kHalfPatch = 15;   // HALF_PATCH_SIZE, :77

// Candidate / keypoint key: x (12 bits) | y (12 bits) << 12 | score (8 bits) << 24.
// FAST candidates carry coordinates relative to the detection border (x-16, y-16) exactly like the
// reference's vToDistributeKeys (:1159-1160); quadtree outputs keep the same packing.
__host__ __device__ inline uint32_t key_pack(int x, int y, int s) { return (uint32_t)x | ((uint32_t)y << 12) | ((uint32_t)s << 24); }
__host__ __device__ inline int key_x(uint32_t k) { return (int)(k & 0xFFFu); }
__host__ __device__ inline int key_y(uint32_t k) { return (int)((k >> 12) & 0xFFFu); }
__host__ __device__ inline int key_s(uint32_t k) { return (int)(k >> 24); }

struct LevelInfo {
    int w, h, pitch;         // level image size and row pitch (bytes, multiple of 64)
    int off;                 // byte offset of this level inside one image's pyramid block
    float scale, inv_scale;  // mvScaleFactor / mvInvScaleFactor (:478-500)
    int quota;               // mnFeaturesPerLevel (:509-526)
    int patch;               // scaledPatchSize = int(31*scale) (:1184)
    int kp_cap, kp_off;      // capacity / offset of this level in the per-image level-ordered keypoint arrays
    int ncols, nrows, wcell, hcell;   // FAST cell grid (:1087-1095)
    int cell_begin, cell_count;       // this level's cells in the flattened cell table
    int cand_cap, cand_off;  // capacity / offset of this level in the per-image candidate arrays
    int bw, bh;              // detection-area size (maxBorder-minBorder), the quadtree's root extent
    int nini;                // number of quadtree roots = round(bw/bh) (:718)
    float hX;                // root width = bw/nini (:722)
    int xtab_off, ytab_off;  // offsets into the resize coefficient tables (levels >= 1)
    int presort_depth;       // quadtree: keys are counting-sorted by (root, first presort_depth child digits) up front
    int qt_threads;          // quadtree: threads of the workgroup that work on this level (256, or 1024 for the large levels)
};

struct CellInfo {
    int16_t level;
    int16_t x0, y0, x1, y1;  // detectable interior of the cell window in level coordinates
    int16_t _pad;
    int slot_off;            // first candidate slot of this cell inside the per-image slot array
};

// Resize coefficient entry: source index + two 11-bit fixed-point weights (a0 | a1 << 16).
struct ResizeTap { int ofs; int w; };

// k_pyramid_fused: what one tile column (or row) of the top level computes and owns at one level: region [a, b) (for columns a and b are
// multiples of 4), owned interval [o0, o1).  Index: tile * nlevels + level; level 0 carries the window to load (nothing of it is written).
struct PyrSpan { int16_t a, b, o0, o1; };
struct PyrTapOffsets { int x[kMaxLevels], y[kMaxLevels], total; };   // first LDS tap entry of a level's region columns / rows (sized for the widest tile)

struct KeyPointRec { float x, y, size, angle, response; int32_t octave, class_id; };   // = OrbxKeyPoint, 28 B

struct BlurTaps { int k[7]; };                       // 7-tap Gaussian, 8-bit fixed point
struct BlurTiles { int begin[kMaxLevels + 1]; };         // first tile (256 cols x 64 rows) of each level in k_blur's grid
// k_frame_pyramid (orbx_set_pyramid_export): level l's (w + 2 edge) x (h + 2 edge) frame at byte `off` of an image's export block, rows `step` bytes
// apart (a multiple of 16), and the first row band of each level in the launch's grid
struct FrameLayout { int off[kMaxLevels], step[kMaxLevels], band[kMaxLevels + 1], edge; };
struct UmaxTab { int u[16]; };                        // circular patch half-widths (src/ORBextractor.cc:542-570)
struct StereoParams { float mbf, mb; int th_high, th_orb; int debug_flags; };   // ORBmatcher::TH_HIGH, (TH_HIGH+TH_LOW)/2

// ---- guided searches (k_search.hip) ----
struct GridParams {                                               // mnMinX, mnMinY, mfGridElementWidthInv/HeightInv (include/Frame.h:250-251)
    float min_x, min_y, gw_inv, gh_inv;
    float inv_sigma2[kMaxLevels];                                 // mvInvLevelSigma2, read by the chi-square gate (AreaQuery::gate == 2) only
};
struct AreaQuery {                                                // one GetFeaturesInArea call + the per-candidate gate
    float x, y, r, ur;
    int min_level, max_level, active, gate;                      // gate: 0 none, 1 right coordinate (ORBmatcher.cc:107-117), 2 Fuse chi-square (:1437-1469)
};
struct FrustumParams {                                            // what Frame::isInFrustum reads of the Frame (src/Frame.cc:667-773)
    float Rcw[9], tcw[3], Ow[3];                                  // mRcw (row-major), mtcw, mOw
    float qcw[4];                                                 // mTcw.unit_quaternion().coeffs() (x, y, z, w): `Tcw * x3Dw` of the LastFrame search (sophus_action.h)
    float cam[8]; int kb8;                                        // mpCamera: pinhole fx, fy, cx, cy or the 8 Kannala-Brandt parameters
    float min_x, max_x, min_y, max_y, mbf;
    float log_scale_factor; int nlevels;                          // mfLogScaleFactor, mnScaleLevels (MapPoint::PredictScale)
    float scale_factors[kMaxLevels];
    float cos_limit;                                              // viewingCosLimit
    // SearchByProjection(Frame, MapPoints) query parameters when the queries are produced on the device
    float th, th_far; int far_points;
    int rig_mode;                                                 // Frame::isInFrustumChecks: store nothing unless every test passes, level -1 when rejected
    int forward, backward;                                        // SearchByProjection(Frame, LastFrame): bForward / bBackward (k_lastframe_queries)
    int debug_flags;                                              // orbx_debug_stereo_flags (tests): bit 4 = matrix form of Tcw * p (sophus_action.h)
};
// orbm_project_points: the geometry in front of GetFeaturesInArea in the projection-type searches (ORBmatcher.cc:495-732, :1325-1675, :1689-1932,
// :1950-2030, :2196-2260) - see OrbmProjection in include/orbx.h (same fields)
struct ProjectParams {
    float q[4], t[3];
    int second; float q2[4], t2[3], s2;
    float Ow[3];
    int dist_mode, depth_test, camera_type; float cam[8]; int inline_pinhole;
    float min_x, max_x, min_y, max_y; int bounds_mode;
    int distance_test, angle_test;
    float bf;
};
// The points ONE frame of a batched tracking search is matched against: the arrays of the resident set it names and its size, where the frame's rows
// start in everything the batch lays out per point (`offset`: queries, track x 5, level, in_view, q_start / q_count) and where its rows start in the
// uploaded call-time flags (`flags`: is_bad / has_obs).
//   one set for every frame (orbm_search_local_points_batch / _rig_batch): the same set B times, offset = b * M, flags = 0 - the flags are uploaded once
//   frames with their own maps (.._batch_maps): offset = flags = the prefix sum of M_b
//   projection batches (LastFrame / KeyFrame): desc = the frame's uploaded descriptor rows, M = cap_last, offset = flags = b * cap_last (pos .. max_d unused)
struct FrameMapRec { const float *pos, *normal, *min_d, *max_d; const unsigned long long* desc; int M, offset, flags; };
// The device-resident map (orbm_map): the store of map-point fields by slot; state[slot]: bit 0 = the slot holds a point, bit 1 = that point is bad
struct MapStore { unsigned long long* desc; float *pos, *normal, *min_d, *max_d; uint8_t* state; };
constexpr int kMapPresent = 1, kMapBad = 2;
constexpr int kMapChunk = 256;         // visited positions per workgroup of the local-map build: one chunk, one count
// one visited key-frame row of a local-map build (Tracking::UpdateLocalPoints): `n` slots of row `row`, which frame `set` visits at positions
// [pos0, pos0 + n) of its walk; the row's chunks are chunk0 .. chunk0 + ceil(n / kMapChunk) - 1 of the call (numbered frame by frame, in visiting order)
struct MapSeg { int set, row, n, pos0, chunk0; };
// one point set the map builds: where its M points go, slot by slot (slots: which store slot point j is; seen: 1 = the slot is in set `set`'s seen list)
struct MapSetRec { int* slots; uint8_t* seen; unsigned long long* desc; float *pos, *normal, *min_d, *max_d; int M, set; };
// the rows of one frame of a map-fed projection batch (k_map_rows_gather), key-frame form: the key frame's row of slots in the map and the keypoints of
// the same key frame, resident (pKF->mvKeysUn[i].angle is read); n: the row's length.  flag record of k_map_row_flags: {row, n, offset into the flag block,
// rule: kRowHoldsGoodPoint = the slot holds a point that is not bad (`!pMP || pMP->isBad()`), kRowHoldsPoint = the slot holds a point, its bad flag is not read}
struct MapRowRec { const int* slots; const KeyPointRec* kps; };
struct MapRowFlagRec { int row, n, off, rule; };
constexpr int kRowHoldsGoodPoint = 0, kRowHoldsPoint = 1;
// one frame of a batched SearchLocalPoints on the map's own sets (orbm_search_local_points_batch_map / _rig_batch_map): the seen bytes and the slot list
// of its set where the build left them, the set's M, and where the frame's rows start in the batch's flag blocks (the prefix sum of M_b)
struct SetFlagRec { const uint8_t* seen; const int* slots; int M, off; };
// one target of a Fuse / Sim3 projection batch fed from the map (orbm_fuse_candidates_batch_map / orbm_search_by_projection_sim3_batch_map): the n slots
// that exclude a point of the set from this target start at entry `off` of the call's list block - the map's rows (Fuse: the whole row of the target's key
// frame, off = row * kf_row_cap) or the uploaded found lists (Sim3); feat0: the row entry of the target's feature 0 (k_fuse_kf_slots reads off + feat0 + bestIdx)
struct MapSkipRec { long long off; int n, feat0; };
constexpr int kSkipTargets = 16;       // targets one thread of k_map_set_table / k_map_skip_dups writes the flag of its position for
// the compacted pair list of a Fuse batch (k_fuse_pairs): a chunk is kPairChunk positions of one target (one workgroup, one count), a tile kPairTile chunks
// (one wave of the scan).  The list is records of `fields` ints - {position, feature} and then best_dist, the position's map slot, pKF->GetMapPoint(feature)
// as a slot, each at the index named here or -1 = not asked for
constexpr int kPairChunk = 256, kPairTile = 64;
struct FusePairOut { int* rec; int fields, dist, point_slot, kf_slot; };
// one map point of orbm_distinctive_descriptors_resident (k_distinctive_resident): its observations are entries [start, start + n) of the call's
// observation table (n >= 1: points without observations are not launched); store: the descriptor of its slot in the map's store (nullptr: not written)
struct DistinctiveRec { unsigned long long* store; int start, n; };
constexpr int kDistinctiveRegMax = 64, kDistinctiveMax = 1024;      // most observations of the register form (one per lane) and of a point at all
// one record of k_grid_build_kfs: the grid of one device-resident key frame (orbm_keyframe) for one set of image bounds
struct GridBuildRec { const KeyPointRec* kps; int* cell_of; int* cell_start; int* cell_items; int N; GridParams g; };
// one target of orbm_fuse_candidates_batch (k_fuse_candidates): a resident key frame's arrays and the grid built for the target's bounds, the projection of
// ORBmatcher::Fuse into it (OrbmFuseTarget::spec), what MapPoint::PredictScale reads of the key frame, and mvInvLevelSigma2 in g.inv_sigma2
struct FuseTargetRec {
    const KeyPointRec* kps; const unsigned long long* desc; const float* ur; const int* cell_start; const int* cell_items;
    ProjectParams P; GridParams g;
    int N, nlevels; float log_scale_factor; float scale_factors[kMaxLevels];
};
// one target of orbm_search_by_projection_sim3_batch (k_sim3_candidates, k_sim3_accept): the Fuse record with no chi-square gate, and where the target's
// row of `vpMatched[idx] != NULL on entry` bytes starts in the uploaded occupancy block (-1: nothing is occupied)
struct Sim3TargetRec { FuseTargetRec F; long long occ_off; };
struct RigRelPose { float q[4], t[3]; };                         // mTrl of a two-camera Frame: unit quaternion coeffs (x, y, z, w), translation
struct VocSlot { int node_id, child_start, child_cnt, word_id; };   // one vocabulary node; children occupy consecutive slots
// Key frame database (orbv_db_*): where the BowVectors of queries sit - query q's sorted word ids / values at ids + start[q] (start == nullptr:
// q * stride), its word count at n[q * n_step] (a host CSR, or the results of the vocabulary transform left on the device)
struct KfdbQuerySet { const uint32_t* ids; const double* vals; const int* start; int stride; const int* n; int n_step; };
// one sharing key of one query, in first-appearance order: its word count, whether it is scored, its score (TemplatedVocabulary::score)
constexpr int kKfdbRecsPerBlock = 32;       // k_kfdb_count: records per workgroup (4 waves, 8 records each): the query's ids are loaded once per 32
struct KfdbHit { unsigned long long key; double score; int words, scored; };
struct BowItem { int idx1, start2, cnt2, out_off; };
struct BowParams {
    float F12[9];            // fundamental matrix, row-major (Pinhole::epipolarConstrain)
    float ep[2];             // epipole of KF1's centre in KF2
    float scale2[kMaxLevels], sigma2_2[kMaxLevels];
    int only_stereo, coarse, th_low;
    // Kannala-Brandt cameras (KannalaBrandt8::epipolarConstrain = TriangulateMatches > 1e-4): kb8 != 0
    int kb8, nleft1, nleft2;                 // NLeft of the two key frames (-1: one camera)
    float sigma2_1[kMaxLevels];              // mvLevelSigma2 of KF1
    float cam1[2][8], cam2[2][8];            // mvParameters of mpCamera / mpCamera2 of KF1 and KF2
    float R[4][9], t[4][3];                  // relative pose by [bRight1 * 2 + bRight2] (Tll, Tlr, Trl, Trr); one camera: entry 0
};
// Device-resident arrays of one key frame / frame (orbm_keyframe): what the vocabulary-bucket searches read of it, uploaded once.
struct ResidentKF {
    const KeyPointRec* kps; const unsigned long long* desc; const float* ur;
    const uint32_t* node_id;     // mFeatVec as CSR: node ids (ascending), fv_nodes + 1 offsets, feature indices
    const int* fv_start; const int* fv_feat;
    const int* node_of_feat;     // feature -> index of its node in node_id (-1: in no node)
    int N, fv_nodes;
};
struct SftNeighbour { ResidentKF k2; BowParams P; int mp2_off; int _pad; };        // one neighbour of orbm_search_for_triangulation_resident
// one pair of orbm_search_by_bow_resident (offsets into the flag block, -1 = none / all).  k2_nodes_dev != NULL: K2 is a FRAME of the last extraction
// whose FeatureVector the vocabulary transform left on the device; its node count is read there (orbm_search_by_bow_frames_batch)
struct BowPairResident { ResidentKF k1, k2; int mp1_off, elig2_off; const int* k2_nodes_dev; };
// one pair of orbm_search_by_bow_rig_batch: m.k2 = rig frame (descriptors and FeatureVector of the rig transform, m.k2.kps = camera 1's keypoints),
// kps_r = camera 2's keypoints, nleft = Nleft on the device
struct BowPairRig { BowPairResident m; const KeyPointRec* kps_r; const int* nleft; };
// one key frame of orbm_keyframe_create_extracted / _rig_extracted (k_keyframe_counts, k_keyframe_snapshot): where a frame of the last extraction and its
// FeatureVector sit on the device, and the block of the new key frame.  kps / n_l: the frame's (camera 1's) keypoints and their count; kps_r / n_r: camera 2's
// of a rig frame (nullptr: one camera); desc: its descriptor rows (a rig's: the joined rows of the rig transform); ur: nullptr = every entry -1;
// node_id == nullptr: no FeatureVector, else fv_nodes names its node count.  dst: the sections of ResidentKF at the o_* byte offsets (kps at 0);
// N / nn / nf: features, nodes and FeatureVector entries as k_keyframe_counts reported them; angle: the keypoints' angles, packed, for the host's copy.
struct KfSnapRec {
    const KeyPointRec *kps, *kps_r; const int *n_l, *n_r;
    const unsigned long long* desc; const float* ur;
    const uint32_t* node_id; const int* fv_start; const int* fv_feat; const int* fv_nodes;
    uint8_t* dst; float* angle;
    unsigned o_desc, o_ur, o_nid, o_st, o_ft, o_nof;
    int N, nn, nf, cap;
};
// one frame of orbm_map_stereo_points (k_map_stereo_select, k_map_stereo_write): mvKeysUn, mvDepth and the descriptor rows of an image of the last
// extraction and its feature count where the extractor and the depth producer left them; keeps_off: where the frame's `keeps` bytes start in the call's
// staged block (-1: no feature keeps a point); free_off: where its free slots start in the staged slot list; the frame's list of created features is
// feat_all + b * cap (creation order: phase 1 writes it, phase 2 reads it); row: the key-frame row that receives the slots, or -1
struct StereoPointsRec {
    const KeyPointRec* kps; const float* depth; const unsigned long long* desc; const int* n;
    long long keeps_off; int free_off, row;
    float Rwc[9], Ow[3];
};
// what every frame of the call shares: Frame::cx, cy, invfx, invfy, mThDepth, the loop's point count (100), which MapPoint constructor is followed
// (0: key-frame points, 1: temporal points), mvScaleFactors with its last entry apart (a lane indexes the table by its keypoint's octave), the keypoint
// capacity of an image and the keys the LDS sort was given room for (a power of two)
struct StereoPointsParams { float cx, cy, invfx, invfy, th_depth; int max_points, mode, nlevels, cap, sort_cap; float scale_top; float scale[kMaxLevels]; };
constexpr int kStereoPointsSortMax = 16384;    // keys of 8 bytes: 128 KB of gfx950's 160 KB of LDS, the largest power of two that fits
struct KB8StereoParams {                     // Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1530-1587)
    float cam1[8], cam2[8];                  // mpCamera, mpCamera2
    float R12[9], t12[3];                    // mRlr, mtlr
    float sigma2[kMaxLevels];                // mvLevelSigma2
};
#ifdef ORBX_EMU
struct int2 { int x, y; };
struct int4 { int x, y, z, w; };
#endif

// quadtree node, 24 B, lives in LDS
struct QNode {
    int16_t x0, y0, x1, y1;
    uint32_t start;     // first key of this node's span in the key buffers
    uint32_t cnt_buf;   // bits 0..29 key count, bit 30 = which key buffer (0:A 1:B) holds the span
    uint32_t code;      // path from the root: root index, then one base-4 digit (child n1..n4) per level
    uint32_t depth;     // number of digits; while depth < the level's presort depth the span is already ordered by the next digit
};

}  // namespace orbx
