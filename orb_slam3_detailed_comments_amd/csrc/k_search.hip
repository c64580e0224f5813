// k_search.hip — candidate generation + Hamming evaluation for the guided searches of ORBmatcher:
//   k_grid_build   Frame::AssignFeaturesToGrid / PosInGrid (src/Frame.cc:469-504, :962-978): 64x48 bucket grid as CSR,
//                  items in insertion (= index) order inside a cell
//   k_area_search  Frame::GetFeaturesInArea (src/Frame.cc:859-951) fused with the per-candidate part of
//                  ORBmatcher::SearchByProjection (src/ORBmatcher.cc:45-239 and :1950-2184): one wave64 per query
//                  (map point / last-frame point); emits, in GetFeaturesInArea order (cells ix-major, iy-minor, items in
//                  insertion order), every candidate that passes the level / box / right-coordinate gates together with
//                  its Hamming distance and octave.  The order-dependent acceptance loop ("skip keypoints that already
//                  hold a MapPoint with observations", best / second-best / ratio, rotation histogram) is replayed on the
//                  host over these lists (orbm_search.cpp), because an assignment made for one map point removes that
//                  keypoint from the candidate set of every later one (a true sequential dependency).
//   k_fuse_candidates  the candidate search of ORBmatcher::Fuse (src/ORBmatcher.cc:1325-1660) for one resident point set against many resident key
//                  frames: one thread per (point, key frame), geometry, PredictScale, window walk, gates, Hamming distance and the minimum in one pass
//   k_sim3_candidates / k_sim3_accept  ORBmatcher::SearchByProjection(pKF, Scw, ..) (src/ORBmatcher.cc:495-732) for one resident point set from many resident
//                  key frames: the choice of every (point, key frame) against the occupancy on entry, then the sequential accept loop, one wave per key frame
//   k_bow_search   inner loops of ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:1045-1323): one wave per
//                  unmatched feature of KF1 against the features of KF2 in the same vocabulary node.
//   k_map_*        the device-resident map (orbm_map): scatter of updated map points into the store, and Tracking::UpdateLocalPoints
//                  (src/Tracking.cc:4088-4120) for a batch of frames: first occurrence by atomic max, ordered compaction by chunk ballots, field gather
#include "orbx_types.h"
#include "orbx_block.h"
#include "orbx_kernels.h"
#include "kb8_model.h"
#include "sophus_action.h"
#include "glibc_logf_model.h"

namespace orbx {

constexpr int kGridSmallCell = 16;                 // k_grid_build: cells up to this size are ordered by their own thread
constexpr int kGridCols = 64, kGridRows = 48;   // FRAME_GRID_COLS / FRAME_GRID_ROWS, include/Frame.h:44-45

// grid (1), kGridThreads threads.  cell_of: scratch [N] ints.  cell_start: [64*48+1].  Cell id = ix*48 + iy.
// One workgroup because the histogram and the cursors live in LDS; 1024 threads so that a frame's keypoints take one trip per step (the
// kernel is a chain of dependent round trips, not work).
// Batched form (grid = B frames of an extractor's device-resident outputs): n_per_frame != NULL gives N per frame and frame b's arrays sit at
// kps + b * frame_stride, cell_of / cell_items + b * frame_stride, cell_start + b * kGridCellStride.
// Table form (k_grid_build_kfs, grid = records): the grids of device-resident key frames (orbm_keyframe) - separate allocations, each with its own
// keypoints, size, grid constants and outputs (GridBuildRec).
__device__ __forceinline__ void grid_build_body(const KeyPointRec* __restrict__ kps, int N, const GridParams& g, int* __restrict__ cell_of,
                                                int* __restrict__ cell_start, int* __restrict__ cell_items) {
    __shared__ int s_hist[kGridCols * kGridRows];
    __shared__ int s_chunk[256];
    __shared__ unsigned long long s_scan[20];
    const int tid = (int)threadIdx.x;
    constexpr int ncell = kGridCols * kGridRows, NT = kGridThreads, kKeep = 4;
    for (int c = tid; c < ncell; c += NT) s_hist[c] = 0;
    if (tid == 0) s_chunk[0] = 0;                                 // set when a cell is crowded (the ordered chunk placement below then runs)
    __syncthreads();
    int myc[kKeep];                                               // cells of this thread's first keypoints (tid, tid + NT, ..)
#pragma unroll
    for (int k = 0; k < kKeep; k++) myc[k] = -1;
#pragma unroll
    for (int k = 0; k < kKeep; k++) {
        const int i = tid + k * NT;
        if (i < N) {
            const KeyPointRec kp = kps[i];
            const int px = (int)roundf(__fmul_rn(__fsub_rn(kp.x, g.min_x), g.gw_inv));
            const int py = (int)roundf(__fmul_rn(__fsub_rn(kp.y, g.min_y), g.gh_inv));
            if (!(px < 0 || px >= kGridCols || py < 0 || py >= kGridRows)) { myc[k] = px * kGridRows + py; atomicAdd(&s_hist[myc[k]], 1); }
            cell_of[i] = myc[k];
        }
    }
    for (int i = tid + kKeep * NT; i < N; i += NT) {
        const KeyPointRec kp = kps[i];
        const int px = (int)roundf(__fmul_rn(__fsub_rn(kp.x, g.min_x), g.gw_inv));
        const int py = (int)roundf(__fmul_rn(__fsub_rn(kp.y, g.min_y), g.gh_inv));
        int c = -1;
        if (!(px < 0 || px >= kGridCols || py < 0 || py >= kGridRows)) { c = px * kGridRows + py; atomicAdd(&s_hist[c], 1); }
        cell_of[i] = c;
    }
    __syncthreads();
    // exclusive scan of the histogram -> cell_start; s_hist becomes the running cursor of each cell
    // (a thread takes ncell / NT = 3 consecutive cells, so one workgroup scan does)
    {
        constexpr int kPer = ncell / NT;
        static_assert(kPer * NT == ncell, "grid cells per thread");
        int loc[kPer], sum = 0, mx = 0;
#pragma unroll
        for (int k = 0; k < kPer; k++) { const int v = s_hist[tid * kPer + k]; loc[k] = sum; sum += v; mx = v > mx ? v : mx; }
        if (mx > kGridSmallCell) s_chunk[0] = 1;                  // (benign race: every writer stores 1)
        unsigned long long tot;
        const int ex = (int)block_excl_scan<unsigned long long>((unsigned long long)sum, &tot, s_scan);
#pragma unroll
        for (int k = 0; k < kPer; k++) { cell_start[tid * kPer + k] = ex + loc[k]; s_hist[tid * kPer + k] = ex + loc[k]; }
        if (tid == 0) cell_start[ncell] = (int)tot;
        __syncthreads();
        if (s_chunk[0] == 0) {
            // the usual frame: no cell holds more than kGridSmallCell keypoints.  Unordered placement through the LDS cursors, then every
            // thread puts the (few) items of each of its cells into index order = the order of the reference's push_back loop (src/Frame.cc:488-503)
#pragma unroll
            for (int k = 0; k < kKeep; k++) if (myc[k] >= 0) cell_items[atomicAdd(&s_hist[myc[k]], 1)] = tid + k * NT;
            for (int i = tid + kKeep * NT; i < N; i += NT) {
                const int c = cell_of[i];
                if (c >= 0) cell_items[atomicAdd(&s_hist[c], 1)] = i;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kPer; k++) {
                const int st = ex + loc[k], cnt = s_hist[tid * kPer + k] - st;
                for (int a2 = 1; a2 < cnt; a2++) {                // insertion sort of <= kGridSmallCell indices
                    const int v = cell_items[st + a2];
                    int j = a2 - 1;
                    while (j >= 0 && cell_items[st + j] > v) { cell_items[st + j + 1] = cell_items[st + j]; j--; }
                    cell_items[st + j + 1] = v;
                }
            }
            return;
        }
    }
    __syncthreads();
    // crowded cells: stable placement, 256 keypoints at a time in index order (the first four waves work, the others keep the barriers company)
    for (int i0 = 0; i0 < N; i0 += 256) {
        const int i = i0 + tid;
        const int c = (tid < 256 && i < N) ? cell_of[i] : -1;
        if (tid < 256) s_chunk[tid] = c;
        __syncthreads();
        int before = 0, after = 0, cur = 0;
        if (c >= 0) {
            for (int t = 0; t < 256; t++) { const int m = (s_chunk[t] == c); before += (t < tid) & m; after += (t > tid) & m; }
            cur = s_hist[c];
        }
        __syncthreads();
        if (c >= 0) {
            cell_items[cur + before] = i;
            if (after == 0) s_hist[c] = cur + before + 1;     // the last lane of this cell in the chunk advances the cursor
        }
        __syncthreads();
    }
}
__global__ void __launch_bounds__(kGridThreads) k_grid_build(const KeyPointRec* __restrict__ kps, int N, GridParams g,
                                                             int* __restrict__ cell_of, int* __restrict__ cell_start,
                                                             int* __restrict__ cell_items, const int* __restrict__ n_per_frame, int frame_stride) {
    if (n_per_frame) {
        const size_t b = blockIdx.x;
        N = n_per_frame[b]; kps += b * (size_t)frame_stride; cell_of += b * (size_t)frame_stride; cell_items += b * (size_t)frame_stride;
        cell_start += b * (size_t)kGridCellStride;
    }
    grid_build_body(kps, N, g, cell_of, cell_start, cell_items);
}
__global__ void __launch_bounds__(kGridThreads) k_grid_build_kfs(const GridBuildRec* __restrict__ recs) {
    const GridBuildRec& R = recs[blockIdx.x];                      // by reference: the record stays in global memory (scalar loads)
    grid_build_body(R.kps, R.N, R.g, R.cell_of, R.cell_start, R.cell_items);
}

// level filter (with the reference's bCheckLevels quirk, :908), box test (:944) and right-coordinate gate
// (ORBmatcher.cc:107-117 / :2043-2050) of one keypoint against one query
__device__ __forceinline__ bool area_accept(const AreaQuery& A, const KeyPointRec& k, int idx, bool check_levels,
                                            int gate_right, const float* __restrict__ u_right) {
    if (check_levels) {
        if (k.octave < A.min_level) return false;
        if (A.max_level >= 0 && k.octave > A.max_level) return false;
    }
    if (!(fabsf(__fsub_rn(k.x, A.x)) < A.r && fabsf(__fsub_rn(k.y, A.y)) < A.r)) return false;
    if (gate_right && A.gate == 1) {       // (gate 2 = Fuse's chi-square test, which has no radius test on the right coordinate: src/ORBmatcher.cc:1437-1469)
        const float ur = u_right[idx];
        if (ur > 0 && fabsf(__fsub_rn(A.ur, ur)) > A.r) return false;
    }
    return true;
}
// reprojection gate of ORBmatcher::Fuse (src/ORBmatcher.cc:1437-1469): e2 * invSigma2[octave] > 7.8 (stereo keypoint, 3 dof)
// or > 5.99 (monocular, 2 dof), float product compared as double like the reference's float-vs-double-literal comparison
__device__ __forceinline__ bool chi2_accept(const AreaQuery& A, const KeyPointRec& k, float ur, const GridParams& g) {
    const float ex = __fsub_rn(A.x, k.x), ey = __fsub_rn(A.y, k.y);
    float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
    const float inv = g.inv_sigma2[k.octave & (kMaxLevels - 1)];
    if (ur >= 0) {
        const float er = __fsub_rn(A.ur, ur);
        e2 = __fadd_rn(e2, __fmul_rn(er, er));
        return !((double)__fmul_rn(e2, inv) > 7.8);
    }
    return !((double)__fmul_rn(e2, inv) > 5.99);
}

// One wave per query.  grid (ceil(Q / kAreaWaves)), 64 * kAreaWaves threads.  Lane l of a chunk owns window cell l (cells enumerated ix-major,
// iy-minor like the reference's loops): pass 0 counts, the workgroup reserves the spans of its queries in the entry pool with ONE atomicAdd
// (thousands of same-address atomics, one per query, were most of this kernel's time), pass 1 re-enumerates and writes each lane's
// candidates at its ordered offset (wave prefix sum).
// entries: int2 per candidate {idx, dist | octave << 16}; q_start/q_count: CSR; pool_counter: running allocation.
__global__ void __launch_bounds__(64 * kAreaWaves) k_area_search(const AreaQuery* __restrict__ queries, const unsigned long long* __restrict__ qdesc, int Q,
                                                     const KeyPointRec* __restrict__ kps, const float* __restrict__ u_right,
                                                     const unsigned long long* __restrict__ fdesc, GridParams g,
                                                     const int* __restrict__ cell_start, const int* __restrict__ cell_items,
                                                     int gate_right, int* __restrict__ pool_counter, int pool_cap,
                                                     int* __restrict__ q_start, int* __restrict__ q_count, int2* __restrict__ entries) {
    __shared__ int s_cnt[kAreaWaves], s_base;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int q = (int)blockIdx.x * kAreaWaves + wave;
    AreaQuery A{};
    if (q < Q) A = queries[q];
    int cnt_total = 0, start = 0;
    // window of grid cells, src/Frame.cc:877-903
    const int nMinX = imax(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(A.x, g.min_x), A.r), g.gw_inv)));
    const int nMaxX = imin(kGridCols - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(A.x, g.min_x), A.r), g.gw_inv)));
    const int nMinY = imax(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(A.y, g.min_y), A.r), g.gh_inv)));
    const int nMaxY = imin(kGridRows - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(A.y, g.min_y), A.r), g.gh_inv)));
    const bool window_ok = q < Q && A.active && !(nMinX >= kGridCols || nMaxX < 0 || nMinY >= kGridRows || nMaxY < 0) && nMaxX >= nMinX && nMaxY >= nMinY;
    const int ny = nMaxY - nMinY + 1, ncw = window_ok ? (nMaxX - nMinX + 1) * ny : 0;
    const bool check_levels = (A.min_level > 0) || (A.max_level >= 0);
    unsigned long long d0 = 0, d1 = 0, d2 = 0, d3 = 0;
    if (window_ok) { const unsigned long long* dq = qdesc + 4 * (size_t)q; d0 = dq[0]; d1 = dq[1]; d2 = dq[2]; d3 = dq[3]; }
    {
        for (int pass = 0; pass < 2; pass++) {
            if (pass == 1 && cnt_total == 0) break;
            int base = 0;
            for (int c0 = 0; c0 < ncw; c0 += 64) {
                const int c = c0 + lane;
                int s = 0, e = 0;
                if (c < ncw) {
                    const int ix = nMinX + c / ny, iy = nMinY + c % ny;
                    s = cell_start[ix * kGridRows + iy]; e = cell_start[ix * kGridRows + iy + 1];
                }
                int cnt = 0;
                for (int j = s; j < e; j++) {
                    const int idx = cell_items[j];
                    const KeyPointRec k = kps[idx];
                    cnt += (area_accept(A, k, idx, check_levels, gate_right, u_right) && (A.gate != 2 || chi2_accept(A, k, u_right[idx], g))) ? 1 : 0;
                }
                const int incl = wave_incl_scan(cnt);
                if (pass == 1 && start >= 0) {
                    int pos = start + base + incl - cnt;
                    for (int j = s; j < e; j++) {
                        const int idx = cell_items[j];
                        const KeyPointRec k = kps[idx];
                        if (!area_accept(A, k, idx, check_levels, gate_right, u_right)) continue;
                        if (A.gate == 2 && !chi2_accept(A, k, u_right[idx], g)) continue;
                        const unsigned long long* df = fdesc + 4 * (size_t)idx;
                        const int dist = __popcll(d0 ^ df[0]) + __popcll(d1 ^ df[1]) + __popcll(d2 ^ df[2]) + __popcll(d3 ^ df[3]);
                        int2 ent; ent.x = idx; ent.y = dist | (k.octave << 16);
                        entries[pos++] = ent;
                    }
                }
                base += __shfl(incl, 63);
            }
            if (pass == 0) {
                cnt_total = base;
                // one reservation per workgroup: the waves' spans follow each other in wave order
                if (lane == 0) s_cnt[wave] = cnt_total;
                __syncthreads();
                if (threadIdx.x == 0) {
                    int tot = 0;
                    for (int w = 0; w < kAreaWaves; w++) tot += s_cnt[w];
                    s_base = tot > 0 ? atomicAdd(pool_counter, tot) : 0;
                }
                __syncthreads();
                int off = s_base;
                for (int w = 0; w < wave; w++) off += s_cnt[w];
                start = (off + cnt_total <= pool_cap) ? off : -1;   // -1: pool overflow, the host retries with a bigger pool
            }
        }
    }
    if (lane == 0 && q < Q) { q_start[q] = start < 0 ? 0 : start; q_count[q] = cnt_total; }
}

// Frame::isInFrustum (src/Frame.cc:667-773, one camera) + MapPoint::PredictScale (src/MapPoint.cc:688-731) for M map points, one thread each,
// in the reference's fp32 operation order (Eigen >= 3.3 sums a 3-term product coefficient as a0 + (a1 + a2), sophus_action.h; no fused multiply-adds).  Writes the tracking
// fields the reference stores in the MapPoint (mbTrackInView, mTrackProjX / Y / XR, mTrackDepth, mnTrackScaleLevel, mTrackViewCos) and,
// when `queries` is given, the window query of ORBmatcher::SearchByProjection(Frame, MapPoints) for that point (src/ORBmatcher.cc:53-82).
// F.rig_mode (Frame::isInFrustumChecks, src/Frame.cc:1592-1650, one camera of a two-camera rig; the caller passes that camera's mR, mt, twc
// and parameters): nothing is stored unless the point passes every test, and the level of a rejected point is -1 (:756-757).
// (the body takes the frame's parameters by REFERENCE - the kernel argument itself, or the batch's record in global memory: a copy of the record
// (`F = Fb[b]`) made the struct a private variable, 240 bytes of scratch per thread)
__device__ __forceinline__ void frustum_body(const FrustumParams& F, int i, int M, const float* __restrict__ pos, const float* __restrict__ normal,
                                             const float* __restrict__ min_dist, const float* __restrict__ max_dist, const uint8_t* __restrict__ is_bad,
                                             uint8_t* __restrict__ in_view, float* __restrict__ track, int* __restrict__ scale_level, AreaQuery* __restrict__ queries) {
    const float P0 = pos[3 * i], P1 = pos[3 * i + 1], P2 = pos[3 * i + 2];
    bool ok = true;
    float u = -1.0f, v = -1.0f, xr = 0.0f, depth = 0.0f, vcos = 0.0f; int lvl = 0;
    // Pc = mRcw * P + mtcw
    // (the reference works with the MATRIX here, src/Frame.cc:685; Eigen's 3-term sums are a0 + (a1 + a2), sophus_action.h)
    float Pc[3];
    eig_rt3(F.Rcw, F.tcw, P0, P1, P2, Pc);
    const float x = Pc[0], y = Pc[1], z = Pc[2];
    const float Pc_dist = sqrtf(eig_dot3(x, y, z, x, y, z));
    const float invz = __fdiv_rn(1.0f, z);
    if (z < 0.0f) ok = false;
    float uu = 0.f, vv = 0.f;
    if (ok) {
        if (F.kb8) { KB8Cam c; for (int k = 0; k < 8; k++) c.p[k] = F.cam[k]; const float pc[3] = {x, y, z}; float uv[2]; kb8_project(c, pc, uv); uu = uv[0]; vv = uv[1]; }
        else {                                                        // Pinhole::project, src/CameraModels/Pinhole.cpp:61-68
            uu = __fadd_rn(__fdiv_rn(__fmul_rn(F.cam[0], x), z), F.cam[2]);
            vv = __fadd_rn(__fdiv_rn(__fmul_rn(F.cam[1], y), z), F.cam[3]);
        }
        if (uu < F.min_x || uu > F.max_x) ok = false;
        if (ok && (vv < F.min_y || vv > F.max_y)) ok = false;
    }
    if (ok) {
        if (!F.rig_mode) { u = uu; v = vv; }                          // mTrackProjX / Y are set before the distance tests (:705-706)
        const float maxDistance = __fmul_rn(1.2f, max_dist[i]), minDistance = __fmul_rn(0.8f, min_dist[i]);     // MapPoint.cc:658-671
        const float o0 = __fsub_rn(P0, F.Ow[0]), o1 = __fsub_rn(P1, F.Ow[1]), o2 = __fsub_rn(P2, F.Ow[2]);
        const float dist = sqrtf(eig_dot3(o0, o1, o2, o0, o1, o2));
        if (dist < minDistance || dist > maxDistance) ok = false;
        if (ok) {
            const float dot = eig_dot3(o0, o1, o2, normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]);
            vcos = __fdiv_rn(dot, dist);
            if (vcos < F.cos_limit) ok = false;
        }
        if (ok) {
            // MapPoint::PredictScale (src/MapPoint.cc:714-731): ceil(log(ratio) / mfLogScaleFactor) in FLOAT - std::log(float) = glibc's logf
            // (glibc_logf_model.h, checked against the live libm for every positive float), float division, ceil(float)
            const float ratio = __fdiv_rn(max_dist[i], dist);
            int n = (int)ceilf(__fdiv_rn(glibc_logf_model<false>(ratio), F.log_scale_factor));
            if (n < 0) n = 0; else if (n >= F.nlevels) n = F.nlevels - 1;
            lvl = n;
            u = uu; v = vv;
            xr = __fsub_rn(uu, __fmul_rn(F.mbf, invz));
            depth = Pc_dist;
        }
    }
    in_view[i] = ok ? 1 : 0;
    track[i] = u; track[M + i] = v; track[2 * (size_t)M + i] = xr; track[3 * (size_t)M + i] = depth; track[4 * (size_t)M + i] = vcos;
    scale_level[i] = ok ? lvl : (F.rig_mode ? -1 : 0);
    if (queries) {
        AreaQuery q; q.x = 0; q.y = 0; q.r = 0; q.ur = 0; q.min_level = 0; q.max_level = 0; q.active = 0; q.gate = 0;
        if (ok && !(F.far_points && depth > F.th_far) && !(is_bad && is_bad[i])) {
            float r = (double)vcos > 0.998 ? 2.5f : 4.0f;             // RadiusByViewingCos, src/ORBmatcher.cc:242-249
            if (F.th != 1.0f) r = __fmul_rn(r, F.th);
            q.x = u; q.y = v; q.r = __fmul_rn(r, pick(F.scale_factors, lvl)); q.ur = xr;
            q.min_level = lvl - 1; q.max_level = lvl; q.active = 1; q.gate = 1;
        }
        queries[i] = q;
    }
}

__global__ void __launch_bounds__(256) k_frustum(FrustumParams F, int M, const float* __restrict__ pos, const float* __restrict__ normal,
                                                 const float* __restrict__ min_dist, const float* __restrict__ max_dist, const uint8_t* __restrict__ is_bad,
                                                 uint8_t* __restrict__ in_view, float* __restrict__ track /* [6][M]: x, y, xr, depth, cos, - */,
                                                 int* __restrict__ scale_level, AreaQuery* __restrict__ queries, int* __restrict__ zero4) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (zero4 && i < 4) zero4[i] = 0;                             // the pool counter of the window search that follows (saves a fill launch)
    if (i >= M) return;
    frustum_body(F, i, M, pos, normal, min_dist, max_dist, is_bad, in_view, track, scale_level, queries);
}

// The batched form (orbm_search_local_points_batch / _batch_maps): blockIdx.y = frame, frame b uses Fb[b], reads the resident set maps[b] names and
// writes at maps[b].offset - its place in everything laid out by the prefix sums of M_b (in_view, level, queries; track at 5 x offset); its is_bad
// row starts at maps[b].flags.  One set for every frame is the table that names it B times: offset = b * M, flags = 0 (the flags are uploaded once).
// grid ((max M_b + 255) / 256, B): the blocks beyond a frame's M_b leave at once.  The table entry is the same for the whole block (an address made
// of blockIdx.y alone): one scalar load, not one per lane.
__global__ void __launch_bounds__(256) k_frustum_batch(const FrustumParams* __restrict__ Fb, const FrameMapRec* __restrict__ maps, const uint8_t* __restrict__ is_bad,
                                                       uint8_t* __restrict__ in_view, float* __restrict__ track, int* __restrict__ scale_level,
                                                       AreaQuery* __restrict__ queries, int* __restrict__ zero4) {
    const size_t b = blockIdx.y;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (zero4 && i < 4 && b == 0) zero4[i] = 0;
    const FrameMapRec T = maps[b];
    if (i >= T.M) return;
    const size_t o = (size_t)T.offset;
    frustum_body(Fb[b], i, T.M, T.pos, T.normal, T.min_d, T.max_d, is_bad + T.flags, in_view + o, track + 5 * o, scale_level + o, queries + o);
}

// The head of the projection-type searches of ORBmatcher (SearchByProjection(Frame, LastFrame) src/ORBmatcher.cc:1993-2010, (Frame, KeyFrame)
// :2228-2256, (KeyFrame, Sim3, ...) :525-560 / :640-690, Fuse :1388-1430 / :1590-1625, SearchBySim3 :1745-1790 / :1830-1875): transform the map
// point, depth test, projection, image test, distance range, viewing angle - one thread per point, the reference's fp32 operation order
// (Sophus' quaternion action for the transform, Eigen's a0 + (a1 + a2) for norms and dot products; no fused multiply-adds).  Which tests run and how the projection is written differ between the reference's
// methods; P says which.  Outputs: valid, u, v, ur = u - bf / z, 1 / z, dist (the argument of MapPoint::PredictScale, which stays with the
// caller's MapPoint).  skip[i] != 0: the caller's own tests (bad, already matched, ...) have rejected the point.
// (the body, shared with k_fuse_candidates: point (P0, P1, P2) with normal Pn - read with the angle test only - and distance limits [min_inv, max_inv] - compared
// with the distance test only; P by reference: the kernel argument itself or a record in global memory)
__device__ __forceinline__ bool project_point(const ProjectParams& P, float P0, float P1, float P2, const float* __restrict__ Pn, float min_inv, float max_inv,
                                              int debug_flags, float& u, float& v, float& ur, float& invz, float& dist) {
    bool ok = true;
    float pc[3];
    if (debug_flags & 16) se3_act_matrix_form(P.q, P.t, P0, P1, P2, pc);       // test switch: round 3's R * p + t
    else se3_act(P.q, P.t, P0, P1, P2, pc);                       // Tcw * p3Dw: Sophus' quaternion action (so3.hpp:357-367, se3.hpp:321-324)
    if (P.second == 1) sim3_act(P.q2, P.s2, P.t2, pc[0], pc[1], pc[2], pc);       // S21 * p3Dc1 (rxso3.hpp:265-273, sim3.hpp:226-229)
    else if (P.second == 2) se3_act(P.q2, P.t2, pc[0], pc[1], pc[2], pc);         // GetRelativePoseTrl() * x3Dc
    const float x = pc[0], y = pc[1], z = pc[2];
    invz = __fdiv_rn(1.0f, z);
    if (P.depth_test == 1 && z < 0.0f) ok = false;
    if (P.depth_test == 2 && invz < 0.0f) ok = false;
    if (ok) {
        if (P.camera_type == 1) { KB8Cam c; for (int k = 0; k < 8; k++) c.p[k] = P.cam[k]; const float pc[3] = {x, y, z}; float uv[2]; kb8_project(c, pc, uv); u = uv[0]; v = uv[1]; }
        else if (P.inline_pinhole) {                              // x = X * invz; u = fx * x + cx (the hand-written form, e.g. :656-660)
            u = __fadd_rn(__fmul_rn(P.cam[0], __fmul_rn(x, invz)), P.cam[2]);
            v = __fadd_rn(__fmul_rn(P.cam[1], __fmul_rn(y, invz)), P.cam[3]);
        } else {                                                  // Pinhole::project, src/CameraModels/Pinhole.cpp:61-68
            u = __fadd_rn(__fdiv_rn(__fmul_rn(P.cam[0], x), z), P.cam[2]);
            v = __fadd_rn(__fdiv_rn(__fmul_rn(P.cam[1], y), z), P.cam[3]);
        }
        if (P.bounds_mode == 0) { if (u < P.min_x || u > P.max_x || v < P.min_y || v > P.max_y) ok = false; }        // Frame: :2003-2006
        else if (P.bounds_mode == 1 && !(u >= P.min_x && u < P.max_x && v >= P.min_y && v < P.max_y)) ok = false;      // KeyFrame::IsInImage; 2: no image test
    }
    if (ok) {
        ur = __fsub_rn(u, __fmul_rn(P.bf, invz));
        const float o0 = __fsub_rn(P0, P.Ow[0]), o1 = __fsub_rn(P1, P.Ow[1]), o2 = __fsub_rn(P2, P.Ow[2]);
        if (P.dist_mode == 0) dist = sqrtf(eig_dot3(o0, o1, o2, o0, o1, o2));        // PO.norm(): Eigen reduction, a0 + (a1 + a2)
        else dist = sqrtf(eig_dot3(x, y, z, x, y, z));
        if (P.distance_test && (dist < min_inv || dist > max_inv)) ok = false;
        if (ok && P.angle_test) {                                 // PO.dot(Pn) < 0.5 * dist3D
            const float dot = eig_dot3(o0, o1, o2, Pn[0], Pn[1], Pn[2]);
            if (dot < __fmul_rn(0.5f, dist)) ok = false;
        }
    }
    return ok;
}
__global__ void __launch_bounds__(256) k_project_points(ProjectParams P, int M, const float* __restrict__ pos, const float* __restrict__ normal,
                                                        const float* __restrict__ min_inv, const float* __restrict__ max_inv, const uint8_t* __restrict__ skip,
                                                        uint8_t* __restrict__ valid, float* __restrict__ out /* [5][M]: u, v, ur, 1/z, dist */, int debug_flags) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= M) return;
    bool ok = !(skip && skip[i]);
    float u = 0.f, v = 0.f, ur = 0.f, invz = 0.f, dist = 0.f;
    if (ok) ok = project_point(P, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], normal + 3 * (size_t)i, P.distance_test ? min_inv[i] : 0.0f, P.distance_test ? max_inv[i] : 0.0f,
                               debug_flags, u, v, ur, invz, dist);
    valid[i] = ok ? 1 : 0;
    const size_t Ms = (size_t)M;
    out[i] = u; out[Ms + i] = v; out[2 * Ms + i] = ur; out[3 * Ms + i] = invz; out[4 * Ms + i] = dist;
}

// The head of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1970-2023) for a batch of frames: map point
// i of frame b's last frame -> camera (Tcw * x3Dw), 1 / z < 0 rejects, projection, the Frame's image test, radius = th * mvScaleFactors[octave
// of the LAST frame's keypoint], the level window by bForward / bBackward, ur = u - mbf / z for the right-coordinate gate.  grid (capL / 256, B).
// KEYFRAME = true: the head of SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (relocalisation, :2213-2246) instead: no depth
// test, the distance |x3Dw - Ow| must lie in [0.8 mfMinDistance, 1.2 mfMaxDistance] (MapPoint.cc:658-671), the level is MapPoint::PredictScale
// (dist3D, &CurrentFrame) (MapPoint.cc:714-731: glibc's logf, float division, ceil), window [level - 1, level + 1], no right-coordinate gate.
template <bool KEYFRAME>
__device__ __forceinline__ void projection_queries_body(const FrustumParams* __restrict__ Fb, int capL, const int* __restrict__ n_last, const float* __restrict__ pos,
                                                        const uint8_t* __restrict__ valid, const int* __restrict__ octave, const float* __restrict__ min_dist,
                                                        const float* __restrict__ max_dist, AreaQuery* __restrict__ queries, int* __restrict__ zero4) {
    const size_t b = blockIdx.y;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (zero4 && i < 4 && b == 0) zero4[i] = 0;
    if (i >= capL) return;
    const FrustumParams& F = Fb[b];                                // by reference: a private copy would live in scratch memory
    const size_t o = b * (size_t)capL + i;
    AreaQuery q; q.x = 0; q.y = 0; q.r = 0; q.ur = 0; q.min_level = 0; q.max_level = 0; q.active = 0; q.gate = 0;
    if (i < n_last[b] && valid[o]) {
        const float P0 = pos[3 * o], P1 = pos[3 * o + 1], P2 = pos[3 * o + 2];
        float pc[3];
        if (F.debug_flags & 16) se3_act_matrix_form(F.qcw, F.tcw, P0, P1, P2, pc);  // test switch: round 3's R * p + t
        else se3_act(F.qcw, F.tcw, P0, P1, P2, pc);                   // x3Dc = Tcw * x3Dw (:1987, :2224): Sophus' quaternion action, not mRcw * p
        const float x = pc[0], y = pc[1], z = pc[2];
        const float invz = __fdiv_rn(1.0f, z);
        const int oct = KEYFRAME ? 0 : octave[o];
        if (KEYFRAME || (!(invz < 0.0f) && oct >= 0 && oct < F.nlevels)) {
            float u, v;
            if (F.kb8) { KB8Cam c; for (int k = 0; k < 8; k++) c.p[k] = F.cam[k]; const float pcc[3] = {x, y, z}; float uv[2]; kb8_project(c, pcc, uv); u = uv[0]; v = uv[1]; }
            else { u = __fadd_rn(__fdiv_rn(__fmul_rn(F.cam[0], x), z), F.cam[2]); v = __fadd_rn(__fdiv_rn(__fmul_rn(F.cam[1], y), z), F.cam[3]); }
            if (!(u < F.min_x || u > F.max_x || v < F.min_y || v > F.max_y)) {
                if (KEYFRAME) {
                    const float o0 = __fsub_rn(P0, F.Ow[0]), o1 = __fsub_rn(P1, F.Ow[1]), o2 = __fsub_rn(P2, F.Ow[2]);
                    const float dist3D = sqrtf(eig_dot3(o0, o1, o2, o0, o1, o2));                              // PO.norm()
                    const float maxDistance = __fmul_rn(1.2f, max_dist[o]), minDistance = __fmul_rn(0.8f, min_dist[o]);
                    if (!(dist3D < minDistance || dist3D > maxDistance)) {
                        const float ratio = __fdiv_rn(max_dist[o], dist3D);
                        int n = (int)ceilf(__fdiv_rn(glibc_logf_model<false>(ratio), F.log_scale_factor));
                        if (n < 0) n = 0; else if (n >= F.nlevels) n = F.nlevels - 1;
                        q.x = u; q.y = v; q.r = __fmul_rn(F.th, pick(F.scale_factors, n)); q.ur = 0.0f;
                        q.min_level = n - 1; q.max_level = n + 1; q.active = 1; q.gate = 0;
                    }
                } else {
                    q.x = u; q.y = v; q.r = __fmul_rn(F.th, pick(F.scale_factors, oct)); q.ur = __fsub_rn(u, __fmul_rn(F.mbf, invz));
                    if (F.forward) { q.min_level = oct; q.max_level = -1; }
                    else if (F.backward) { q.min_level = 0; q.max_level = oct; }
                    else { q.min_level = oct - 1; q.max_level = oct + 1; }
                    q.active = 1; q.gate = 1;
                }
            }
        }
    }
    queries[o] = q;
}
__global__ void __launch_bounds__(256) k_lastframe_queries(const FrustumParams* __restrict__ Fb, int capL, const int* __restrict__ n_last, const float* __restrict__ pos,
                                                           const uint8_t* __restrict__ valid, const int* __restrict__ octave, AreaQuery* __restrict__ queries,
                                                           int* __restrict__ zero4) {
    projection_queries_body<false>(Fb, capL, n_last, pos, valid, octave, nullptr, nullptr, queries, zero4);
}
__global__ void __launch_bounds__(256) k_keyframe_queries(const FrustumParams* __restrict__ Fb, int capL, const int* __restrict__ n_kf, const float* __restrict__ pos,
                                                          const uint8_t* __restrict__ valid, const float* __restrict__ min_dist, const float* __restrict__ max_dist,
                                                          AreaQuery* __restrict__ queries, int* __restrict__ zero4) {
    projection_queries_body<true>(Fb, capL, n_kf, pos, valid, nullptr, min_dist, max_dist, queries, zero4);
}

// The window search of a BATCH of frames, one THREAD per query (k_area_search spends a wave on a query: right for one frame's few thousand
// queries, which must finish in microseconds; a batch has hundreds of thousands and wants throughput).  A thread walks its window cells in the
// reference's order (ix-major, iy-minor, items in insertion order), counts, the workgroup reserves its span of the entry pool with one
// atomicAdd, and a second walk writes {idx, dist | octave << 16} at the thread's offset.  Same gates as k_area_search.  blockIdx.y = frame.
// On pool overflow nothing is written and the counts are 0 (the host sees the counter, enlarges the pool and repeats).
// Frame b's maps[b].M queries sit at maps[b].offset, their descriptors are maps[b].desc: the resident set of a local map, or the frame's rows of a
// projection batch's upload (M = cap_last, offset = b * cap_last).  grid ((max M_b + 255) / 256, B); a block beyond its frame's M_b leaves before
// the first barrier.
// (the body: queries / q_start / q_count / qdesc / the frame's keypoints and grid are THIS frame's, Q its number of queries)
__device__ __forceinline__ void area_search_threads_body(const AreaQuery* __restrict__ queries, const unsigned long long* __restrict__ qdesc, int Q,
                                                         const KeyPointRec* __restrict__ kps, const float* __restrict__ u_right,
                                                         const unsigned long long* __restrict__ fdesc, const GridParams& g, const int* __restrict__ cell_start,
                                                         const int* __restrict__ cell_items, int gate_right, int* __restrict__ pool_counter, int pool_cap,
                                                         int* __restrict__ q_start, int* __restrict__ q_count, int2* __restrict__ entries) {
    __shared__ int s_scan[20];
    __shared__ int s_base;
    // the first kAreaKeep accepted keypoints of every query (index | octave << 16), [slot][thread]: the second pass - Hamming distances and the
    // writes - then reads them back instead of walking the window, its cells, keypoint records and gates again (round 4; most queries accept fewer)
    constexpr int kAreaKeep = 12;
    __shared__ uint32_t s_keep[kAreaKeep * 256];
    const int q = (int)(blockIdx.x * 256 + threadIdx.x);
    AreaQuery A{};
    if (q < Q) A = queries[q];
    const int nMinX = imax(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(A.x, g.min_x), A.r), g.gw_inv)));
    const int nMaxX = imin(kGridCols - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(A.x, g.min_x), A.r), g.gw_inv)));
    const int nMinY = imax(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(A.y, g.min_y), A.r), g.gh_inv)));
    const int nMaxY = imin(kGridRows - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(A.y, g.min_y), A.r), g.gh_inv)));
    const bool window_ok = q < Q && A.active && !(nMinX >= kGridCols || nMaxX < 0 || nMinY >= kGridRows || nMaxY < 0) && nMaxX >= nMinX && nMaxY >= nMinY;
    const bool check_levels = (A.min_level > 0) || (A.max_level >= 0);
    int cnt = 0;
    if (window_ok) {
        for (int ix = nMinX; ix <= nMaxX; ix++) {
            const int s = cell_start[ix * kGridRows + nMinY], e = cell_start[ix * kGridRows + nMaxY + 1];    // the cells of one column are consecutive
            for (int j = s; j < e; j++) {
                const int idx = cell_items[j];
                const KeyPointRec k = kps[idx];
                if (area_accept(A, k, idx, check_levels, gate_right, u_right) && (A.gate != 2 || chi2_accept(A, k, u_right[idx], g))) {
                    if (cnt < kAreaKeep) s_keep[cnt * 256 + (int)threadIdx.x] = (uint32_t)idx | ((uint32_t)k.octave << 16);
                    cnt++;
                }
            }
        }
    }
    int total;
    const int excl = block_excl_scan<int>(cnt, &total, s_scan);
    if (threadIdx.x == 0) s_base = total > 0 ? atomicAdd(pool_counter, total) : 0;
    __syncthreads();
    const bool fits = s_base + total <= pool_cap;
    const int start = s_base + excl;
    if (window_ok && cnt > 0 && fits) {
        const unsigned long long* dq = qdesc + 4 * (size_t)q;
        const unsigned long long d0 = dq[0], d1 = dq[1], d2 = dq[2], d3 = dq[3];
        int pos = start;
        if (cnt <= kAreaKeep) {
            for (int i = 0; i < cnt; i++) {
                const uint32_t e = s_keep[i * 256 + (int)threadIdx.x];
                const int idx = (int)(e & 0xFFFFu);
                const unsigned long long* df = fdesc + 4 * (size_t)idx;
                const int dist = __popcll(d0 ^ df[0]) + __popcll(d1 ^ df[1]) + __popcll(d2 ^ df[2]) + __popcll(d3 ^ df[3]);
                int2 ent; ent.x = idx; ent.y = dist | (int)(e & 0xFFFF0000u);
                entries[pos++] = ent;
            }
        } else
        for (int ix = nMinX; ix <= nMaxX; ix++) {
            const int s = cell_start[ix * kGridRows + nMinY], e = cell_start[ix * kGridRows + nMaxY + 1];
            for (int j = s; j < e; j++) {
                const int idx = cell_items[j];
                const KeyPointRec k = kps[idx];
                if (!area_accept(A, k, idx, check_levels, gate_right, u_right)) continue;
                if (A.gate == 2 && !chi2_accept(A, k, u_right[idx], g)) continue;
                const unsigned long long* df = fdesc + 4 * (size_t)idx;
                const int dist = __popcll(d0 ^ df[0]) + __popcll(d1 ^ df[1]) + __popcll(d2 ^ df[2]) + __popcll(d3 ^ df[3]);
                int2 ent; ent.x = idx; ent.y = dist | (k.octave << 16);
                entries[pos++] = ent;
            }
        }
    }
    if (q < Q) { q_start[q] = fits ? start : 0; q_count[q] = fits ? cnt : 0; }
}
__global__ void __launch_bounds__(256) k_area_search_threads(const AreaQuery* __restrict__ queries, const FrameMapRec* __restrict__ maps,
                                                             const KeyPointRec* __restrict__ kps, const float* __restrict__ u_right,
                                                             const unsigned long long* __restrict__ fdesc, GridParams g, const int* __restrict__ cell_start,
                                                             const int* __restrict__ cell_items, int gate_right, int* __restrict__ pool_counter, int pool_cap,
                                                             int* __restrict__ q_start, int* __restrict__ q_count, int2* __restrict__ entries, int frame_stride) {
    const size_t b = blockIdx.y, f = b * (size_t)frame_stride;
    const FrameMapRec T = maps[b];
    if ((int)(blockIdx.x * 256) >= T.M) return;
    const size_t o = (size_t)T.offset;
    area_search_threads_body(queries + o, T.desc, T.M, kps + f, u_right + f, fdesc + 4 * f, g, cell_start + b * (size_t)kGridCellStride, cell_items + f, gate_right,
                             pool_counter, pool_cap, q_start + o, q_count + o, entries);
}

// The candidate search of ORBmatcher::Fuse (src/ORBmatcher.cc:1325-1528 with the chi-square gate, :1543-1660 without) for ONE resident point set
// against K resident key frames (orbm_fuse_candidates_batch): one THREAD per (point, key frame), grid ((M + 255) / 256, K).  A Fuse window is 4-9
// grid cells with a handful of keypoints (radius 3-11 px against cells of ~12 x 10 px): a wave per pair would idle 60 lanes, and nothing but the best
// candidate leaves the thread - no candidate lists, no pool.  Both halves in one kernel: the query of a pair (32 bytes) never travels through memory,
// and a pair rejected by the geometry costs its thread nothing further.
//   fuse_query  the head of the reference's loop for one pair: project_point (the body of k_project_points: depth, image, distance and viewing-angle
//               tests, ur = u - bf / z), then MapPoint::PredictScale(dist3D, pKF) (src/MapPoint.cc:688-709) as k_keyframe_queries evaluates it - glibc's
//               logf, float division, ceil, the clamps - and the radius th * mvScaleFactors[level] (:1425-1428 / :1615-1618)
//   fuse_best   KeyFrame::GetFeaturesInArea's window walk in the reference's order (cells ix-major, iy-minor, keypoints in insertion order), per
//               candidate the level gate (octave < level - 1 || octave > level rejects, :1454 / :1638), the chi-square gate (chi2_accept) when the query
//               asks for it, the Hamming distance, a strict `<` minimum - the first candidate in reference order wins a tie
// T[k] is read by reference (blockIdx.y alone forms its address: scalar loads, no private copy of the record).
__device__ __forceinline__ bool fuse_query(const FuseTargetRec& R, int i, const float* __restrict__ pos, const float* __restrict__ normal, const float* __restrict__ min_d,
                                           const float* __restrict__ max_d, float th, int chi2_gate, int debug_flags, AreaQuery& A) {
    const float maxd = max_d[i];
    float u = 0.f, v = 0.f, ur = 0.f, invz = 0.f, dist = 0.f;
    // GetMinDistanceInvariance() = 0.8f * mfMinDistance, GetMaxDistanceInvariance() = 1.2f * mfMaxDistance (src/MapPoint.cc:658-671)
    if (!project_point(R.P, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], normal + 3 * (size_t)i, __fmul_rn(0.8f, min_d[i]), __fmul_rn(1.2f, maxd), debug_flags, u, v, ur,
                       invz, dist)) return false;
    const float ratio = __fdiv_rn(maxd, dist);
    int n = (int)ceilf(__fdiv_rn(glibc_logf_model<false>(ratio), R.log_scale_factor));
    if (n < 0) n = 0; else if (n >= R.nlevels) n = R.nlevels - 1;
    A.x = u; A.y = v; A.r = __fmul_rn(th, pick(R.scale_factors, n)); A.ur = ur;
    A.min_level = n - 1; A.max_level = n; A.active = 1; A.gate = chi2_gate ? 2 : 0;
    return true;
}
// (taken(idx): the keypoint is invisible to this query - ORBmatcher::SearchByProjection(pKF, Scw, ..)'s `if (vpMatched[idx]) continue;`; Fuse has no such test)
template <class Taken>
__device__ __forceinline__ void fuse_best_free(const FuseTargetRec& R, const AreaQuery& A, const unsigned long long* __restrict__ dq, const Taken& taken, int& best_idx,
                                               int& best_dist) {
    const GridParams& g = R.g;
    const int nMinX = imax(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(A.x, g.min_x), A.r), g.gw_inv)));
    const int nMaxX = imin(kGridCols - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(A.x, g.min_x), A.r), g.gw_inv)));
    const int nMinY = imax(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(A.y, g.min_y), A.r), g.gh_inv)));
    const int nMaxY = imin(kGridRows - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(A.y, g.min_y), A.r), g.gh_inv)));
    if (nMinX >= kGridCols || nMaxX < 0 || nMinY >= kGridRows || nMaxY < 0 || nMaxX < nMinX || nMaxY < nMinY) return;
    const unsigned long long d0 = dq[0], d1 = dq[1], d2 = dq[2], d3 = dq[3];
    for (int ix = nMinX; ix <= nMaxX; ix++) {
        const int s = R.cell_start[ix * kGridRows + nMinY], e = R.cell_start[ix * kGridRows + nMaxY + 1];        // the cells of one column are consecutive
        for (int j = s; j < e; j++) {
            const int idx = R.cell_items[j];
            if (taken(idx)) continue;
            const KeyPointRec k = R.kps[idx];
            if (!area_accept(A, k, idx, true, 0, nullptr)) continue;
            if (A.gate == 2 && !chi2_accept(A, k, R.ur[idx], g)) continue;
            const unsigned long long* df = R.desc + 4 * (size_t)idx;
            const int dist = __popcll(d0 ^ df[0]) + __popcll(d1 ^ df[1]) + __popcll(d2 ^ df[2]) + __popcll(d3 ^ df[3]);
            if (dist < best_dist) { best_dist = dist; best_idx = idx; }
        }
    }
}
__device__ __forceinline__ void fuse_best(const FuseTargetRec& R, const AreaQuery& A, const unsigned long long* __restrict__ dq, int& best_idx, int& best_dist) {
    fuse_best_free(R, A, dq, [](int) { return false; }, best_idx, best_dist);
}
// skip: [K][M] bytes or NULL (pairs the caller excludes); best_idx / best_dist: [K][M], -1 where the reference would not fuse (best_dist may be NULL)
__global__ void __launch_bounds__(256) k_fuse_candidates(const FuseTargetRec* __restrict__ T, int M, const float* __restrict__ pos, const float* __restrict__ normal,
                                                         const float* __restrict__ min_d, const float* __restrict__ max_d, const unsigned long long* __restrict__ qdesc,
                                                         const uint8_t* __restrict__ skip, float th, int chi2_gate, int th_low, int debug_flags,
                                                         int* __restrict__ best_idx, int* __restrict__ best_dist) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= M) return;
    const FuseTargetRec& R = T[blockIdx.y];
    const size_t o = (size_t)blockIdx.y * (size_t)M + (size_t)i;
    int bi = -1, bd = 256;                                            // bestDist = 256 (:1443; INT_MAX at :1630 - either is above TH_LOW)
    if (R.N > 0 && !(skip && skip[o])) {
        AreaQuery A;
        if (fuse_query(R, i, pos, normal, min_d, max_d, th, chi2_gate, debug_flags, A)) fuse_best(R, A, qdesc + 4 * (size_t)i, bi, bd);
    }
    if (bd > th_low) bi = -1;                                         // bestDist <= TH_LOW (:1505 / :1654)
    best_idx[o] = bi;
    if (best_dist) best_dist[o] = bi >= 0 ? bd : -1;
}

// ORBmatcher::SearchByProjection(KeyFrame* pKF, Sim3f& Scw, vpPoints, [vpPointsKFs,] vpMatched, [vpMatchedKF,] th, ratioHamming) (src/ORBmatcher.cc:495-606,
// :608-732) for ONE resident point set against K resident key frames, each under its own Sim3 (orbm_search_by_projection_sim3_batch).  The head of the
// reference's loop is Fuse's (fuse_query, no chi-square gate) and so is the window walk (fuse_best_free), but here the loop over the points is sequential:
// a keypoint that is occupied on entry or taken by an earlier point is invisible to every later one, and a point whose best distance is above
// TH_LOW * ratioHamming (`int * float`: a float comparison) takes nothing, so a later point can still have that keypoint.
//   sim3_choice        the keypoint point i takes when the keypoints `taken` names are invisible, or -1.  It is the FIRST minimum of the walk: removing a
//                      keypoint other than that one never changes it, and removing it can only raise the minimum - a point that takes nothing never will
//   k_sim3_candidates  one THREAD per (point, key frame), grid ((M + 255) / 256, K): the choice against the occupancy on entry.  Nothing else leaves the thread
//   k_sim3_accept      one wave per key frame, the occupancy bitmap in LDS: the points in order, 64 at a time, in the optimistic rounds of local_accept_body
__device__ __forceinline__ bool bit_of(const uint32_t* bits, int i) { return ((bits[i >> 5] >> (i & 31)) & 1u) != 0u; }
template <class Taken>
__device__ __forceinline__ int sim3_choice(const FuseTargetRec& R, int i, const float* __restrict__ pos, const float* __restrict__ normal, const float* __restrict__ min_d,
                                           const float* __restrict__ max_d, const unsigned long long* __restrict__ qdesc, float th, float max_dist, int debug_flags,
                                           const Taken& taken) {
    AreaQuery A;
    int bi = -1, bd = 256;                                            // bestDist = 256 (:582 / :698)
    if (fuse_query(R, i, pos, normal, min_d, max_d, th, 0, debug_flags, A)) fuse_best_free(R, A, qdesc + 4 * (size_t)i, taken, bi, bd);
    return (bi >= 0 && (float)bd <= max_dist) ? bi : -1;             // bestDist <= TH_LOW * ratioHamming (:609 / :722)
}
// occupied: the uploaded rows of `vpMatched[idx] != NULL` bytes (target k's at T[k].occ_off); skip: [K][M] bytes or NULL; max_dist = TH_LOW * ratioHamming;
// choice: [K][M]
__global__ void __launch_bounds__(256) k_sim3_candidates(const Sim3TargetRec* __restrict__ T, int M, const float* __restrict__ pos, const float* __restrict__ normal,
                                                         const float* __restrict__ min_d, const float* __restrict__ max_d, const unsigned long long* __restrict__ qdesc,
                                                         const uint8_t* __restrict__ occupied, const uint8_t* __restrict__ skip, float th, float max_dist,
                                                         int debug_flags, int* __restrict__ choice) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= M) return;
    const Sim3TargetRec& S = T[blockIdx.y];
    const size_t o = (size_t)blockIdx.y * (size_t)M + (size_t)i;
    const uint8_t* occ = S.occ_off >= 0 ? occupied + S.occ_off : (const uint8_t*)nullptr;
    int c = -1;
    if (S.F.N > 0 && !(skip && skip[o]))
        c = sim3_choice(S.F, i, pos, normal, min_d, max_d, qdesc, th, max_dist, debug_flags, [occ](int idx) { return occ && occ[idx]; });
    choice[o] = c;
}
// The accept loop.  Per 64 consecutive points, one per lane, until none is pending:
//   1. a lane whose choice has been taken since it was made walks its window again against the live bitmap (the query is recomputed: fuse_query is
//      deterministic, and conflicts are rare) - its choice is then what the sequential loop would pick if every earlier point had been committed;
//   2. every pending lane claims its keypoint (LDS, minimum lane per slot of a small table keyed by the low bits of the index);
//   3. a lane is DIRTY if an earlier lane claims its slot: that lane may take the very keypoint (or one that merely shares the slot - the lane then only
//      waits a round).  A claim on any OTHER keypoint cannot change a first minimum;
//   4. the lanes before the first dirty one commit, the others repeat from 1.  The first pending lane holds the minimum of its slot: every round commits.
// assigned: [K][cap], -1 = untouched - every entry is written once: by the lane that commits it, or after the loop (not occupied then, or occupied on entry);
// dynamic LDS: the occupancy bitmap, (N + 31) / 32 words for the largest N of the call.
constexpr int kSim3ClaimSlots = 256;
__global__ void __launch_bounds__(64) k_sim3_accept(const Sim3TargetRec* __restrict__ T, int M, const float* __restrict__ pos, const float* __restrict__ normal,
                                                    const float* __restrict__ min_d, const float* __restrict__ max_d, const unsigned long long* __restrict__ qdesc,
                                                    const uint8_t* __restrict__ occupied, float th, float max_dist, int debug_flags, int cap,
                                                    const int* __restrict__ choice, int* __restrict__ assigned, int* __restrict__ nmatches) {
    ORBX_DYN_SMEM(smem);
    uint32_t* s_occ = (uint32_t*)smem;
    __shared__ unsigned s_claim[kSim3ClaimSlots];
    const int lane = lane_id();
    const Sim3TargetRec& S = T[blockIdx.x];
    const FuseTargetRec& R = S.F;
    const int N = R.N, nwords = (N + 31) / 32;
    const uint8_t* occ0 = S.occ_off >= 0 ? occupied + S.occ_off : (const uint8_t*)nullptr;
    choice += blockIdx.x * (size_t)M; assigned += blockIdx.x * (size_t)cap;
    for (int w = lane; w < nwords; w += 64) {
        uint32_t bits = 0;
        if (occ0) for (int k = 0; k < 32; k++) { const int i = 32 * w + k; if (i < N && occ0[i]) bits |= 1u << k; }
        s_occ[w] = bits;
    }
    for (int i = lane; i < kSim3ClaimSlots; i += 64) s_claim[i] = 0xFFu;
    ORBX_WAVE_SYNC();
    int nm = 0;
    for (int i0 = 0; i0 < M; i0 += 64) {
        const int qi = i0 + lane;
        int c = qi < M ? choice[qi] : -1;
        bool pending = c >= 0;
        while (__ballot(pending) != 0ull) {
            // 1. a choice that is gone: again, against the live occupancy
            if (pending && bit_of(s_occ, c)) {
                c = sim3_choice(R, qi, pos, normal, min_d, max_d, qdesc, th, max_dist, debug_flags, [s_occ](int idx) { return bit_of(s_occ, idx); });
                pending = c >= 0;
            }
            // 2. claims
            const unsigned slot = (unsigned)c & (unsigned)(kSim3ClaimSlots - 1);
            if (pending) atomicMin(&s_claim[slot], (unsigned)lane);
            ORBX_WAVE_SYNC();
            // 3. dirty: an earlier lane claims my slot
            const bool dirty = pending && s_claim[slot] < (unsigned)lane;
            const unsigned long long dmask = __ballot(dirty);
            const int first_dirty = dmask ? __ffsll(dmask) - 1 : 64;
            ORBX_WAVE_SYNC();
            if (pending) s_claim[slot] = 0xFFu;                         // (every claimer of a slot restores it)
            ORBX_WAVE_SYNC();
            // 4. commit the lanes before the first dirty one
            const bool commit = pending && lane < first_dirty;
            if (commit) { assigned[c] = qi; atomicOr(&s_occ[c >> 5], 1u << (c & 31)); pending = false; }
            nm += __popcll(__ballot(commit));
            ORBX_WAVE_SYNC();
        }
    }
    ORBX_WAVE_SYNC();
    for (int i = lane; i < cap; i += 64) if (i >= N || (occ0 && occ0[i]) || !bit_of(s_occ, i)) assigned[i] = -1;
    if (lane == 0) nmatches[blockIdx.x] = nm;
}

// ---- reference logic that the accept loops and the BoW pruning share ----
// The best and the second best of one candidate window, as the strict `<` tests of the reference leave them (the FIRST candidate with the smallest distance;
// the second best is the smallest among the others).  k1 / k2: keys (dist << 16 | position in the window), 0xFFFFFFFF = none; e1 / e2: the entries' packed
// dist | level << 16; idx: keypoint of the best.  16 bits hold every position and keypoint index: a query's candidates are distinct keypoints of one frame, and
// a frame has fewer than 65535 (kp_total_cap, refused in orbx_api.cpp: configure)
struct BestTwo {
    unsigned k1, k2; int e1, e2, idx;
    __device__ __forceinline__ bool any() const { return k1 != 0xFFFFFFFFu; }
};
// the reference's four variables of a window with a best (any()); no second best: bestDist2 = 256, bestLevel2 = -1
struct BestTwoLevels { int bestDist, bestLevel, bestDist2, bestLevel2; };
__device__ __forceinline__ BestTwoLevels unpack(const BestTwo& r) {
    const bool second = r.k2 != 0xFFFFFFFFu;
    return {r.e1 & 0xFFFF, r.e1 >> 16, second ? (r.e2 & 0xFFFF) : 256, second ? (r.e2 >> 16) : -1};
}
// occupied(keypoint): the candidate is skipped (F.mvpMapPoints[idx] holds a point with observations)
template <typename Occupied>
__device__ __forceinline__ BestTwo best_two_scan(const int2* __restrict__ entries, int st, int cnt, const Occupied& occupied) {
    BestTwo r = {0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, -1};
    for (int k = 0; k < cnt; k++) {
        const int2 e = entries[st + k];
        if (occupied(e.x)) continue;
        const unsigned key = ((unsigned)(e.y & 0xFFFF) << 16) | (unsigned)k;
        if (key < r.k1) { r.k2 = r.k1; r.e2 = r.e1; r.k1 = key; r.e1 = e.y; r.idx = e.x; } else if (key < r.k2) { r.k2 = key; r.e2 = e.y; }
    }
    return r;
}
// rot = angle1 - angle2 [+ 360], bin = round(rot / 30) (src/ORBmatcher.cc:2118-2125 and :396-412; the reference's 1 / HISTO_LENGTH factor)
__device__ __forceinline__ int rot_bin(float angle1, float angle2) {
    float rot = __fsub_rn(angle1, angle2);
    if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
    const int bin = (int)roundf(__fmul_rn(rot, 1.0f / 30));
    return bin == 30 ? 0 : bin;
}
// ComputeThreeMaxima (src/ORBmatcher.cc:2335-2377) over the 30 bin sizes, every lane alike: the three fullest bins, the second / third only while they
// hold at least 10 % of the first (-1: dropped)
struct ThreeMaxima {
    int ind1, ind2, ind3;
    __device__ __forceinline__ bool keeps(int bin) const { return bin == ind1 || bin == ind2 || bin == ind3; }
};
__device__ __forceinline__ ThreeMaxima three_maxima(const int* s_hist) {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < 30; i++) {
        const int sz = s_hist[i];
        if (sz > max1) { max3 = max2; max2 = max1; max1 = sz; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (sz > max2) { max3 = max2; max2 = sz; ind3 = ind2; ind2 = i; }
        else if (sz > max3) { max3 = sz; ind3 = i; }
    }
    if ((float)max2 < __fmul_rn(0.1f, (float)max1)) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < __fmul_rn(0.1f, (float)max1)) ind3 = -1;
    return {ind1, ind2, ind3};
}

// ORBmatcher::SearchByProjection(Frame, MapPoints) accept loop (src/ORBmatcher.cc:62-166) on the device, one wave per frame of a batch.
// The loop is sequential over the map points: a keypoint that has received a map point WITH observations is skipped by every later point.
// Conflicts are rare, so the wave works on 64 consecutive map points at a time, one per lane, optimistically:
//   1. every pending lane walks its candidates against the current occupancy: best / second best exactly as the strict `<` tests of the
//      reference leave them (the FIRST candidate with the smallest distance; the second best is the smallest among the others), decision;
//   2. lanes whose decision occupies a keypoint publish the claim (LDS, minimum lane per keypoint);
//   3. a lane is DIRTY if an earlier lane of this round claims one of its free candidates - its decision may not stand;
//   4. the lanes before the first dirty one commit (their decisions are what the sequential loop produces: nothing earlier touches their
//      candidates), the others repeat from 1 with the new occupancy.  The first pending lane is never dirty, so every round commits.
// F.mvpMapPoints[idx] = pMP without observations does not occupy; a later point may overwrite it: assignments are merged with atomicMax on
// the map point index (the sequential last writer is the largest index).
// Frame b has maps[b].M points; its q_start / q_count rows (LASTFRAME: and last_angle) start at maps[b].offset, its has_obs row at maps[b].flags (one
// set for every frame: offset = b * M, flags = 0; frames with their own maps: both the prefix sum of M_b; a projection batch: both b * cap_last).
// occupied0: [B][cap] bytes or NULL; has_obs: NULL = all observed.  assigned: [B][cap], -1 = untouched; nmatches: [B].
// dynamic LDS: occupancy bitmap ((cap + 31) / 32 words) | claiming lane per keypoint (cap words) | LASTFRAME: one accept event per query (M words).
// LASTFRAME = the accept loop of SearchByProjection(CurrentFrame, LastFrame) (src/ORBmatcher.cc:2025-2150): the best candidate alone decides
// (bestDist <= TH_HIGH, no ratio test), and every accepted pair goes into the rotation histogram
// (:2118-2126, ComputeThreeMaxima :2335-2377): after the loop the pairs outside the three fullest bins are taken back (assigned = -2 = reset to
// NULL, nmatches--) - per accept EVENT, as the reference's rotHist lists are (a keypoint that was given twice has two entries).
template <bool LASTFRAME>
__device__ __forceinline__ void local_accept_body(const FrameMapRec* __restrict__ maps, int cap, const int* __restrict__ n_per_frame, const int* __restrict__ q_start,
                                                  const int* __restrict__ q_count, const int2* __restrict__ entries, const uint8_t* __restrict__ occupied0,
                                                  const uint8_t* __restrict__ has_obs, float nnratio, int th_high, int* __restrict__ assigned,
                                                  int* __restrict__ nmatches, const float* __restrict__ last_angle, const KeyPointRec* __restrict__ cur_kps,
                                                  int check_ori) {
    int* events = nullptr;
    ORBX_DYN_SMEM(smem);
    const int nwords = (cap + 31) / 32;
    uint32_t* s_occ = (uint32_t*)smem;
    unsigned* s_claim = (unsigned*)(smem + 4 * (size_t)nwords);
    __shared__ int s_hist[32];
    const int lane = lane_id();
    const size_t b = blockIdx.x;
    const int N = n_per_frame[b];
    const int M = maps[b].M;
    const size_t qo = (size_t)maps[b].offset;
    q_start += qo; q_count += qo; assigned += b * (size_t)cap;
    if (has_obs) has_obs += maps[b].flags;
    if (LASTFRAME) {
        last_angle += qo; cur_kps += b * (size_t)cap;
        events = (int*)(s_claim + cap);                               // in LDS: written and read by different lanes of this wave, in program order
        if (lane < 32) s_hist[lane] = 0;
    }
    for (int w = lane; w < nwords; w += 64) {
        uint32_t bits = 0;
        if (occupied0) for (int k = 0; k < 32; k++) { const int i = 32 * w + k; if (i < N && occupied0[b * (size_t)cap + i]) bits |= 1u << k; }
        s_occ[w] = bits;
    }
    for (int i = lane; i < cap; i += 64) { assigned[i] = -1; s_claim[i] = 0xFFu; }
    ORBX_WAVE_SYNC();
    int nm = 0;
    for (int i0 = 0; i0 < M; i0 += 64) {
        const int qi = i0 + lane;
        const int cnt = qi < M ? q_count[qi] : 0, st = qi < M ? q_start[qi] : 0;
        const bool obs = qi < M && (!has_obs || has_obs[qi]);
        bool pending = cnt > 0;
        if (LASTFRAME && qi < M) events[qi] = -1;
        while (__ballot(pending) != 0ull) {
            // 1. decision against the current occupancy
            const BestTwo best = best_two_scan(entries, st, pending ? cnt : 0, [&](int i) { return ((s_occ[i >> 5] >> (i & 31)) & 1u) != 0; });
            const int idx1 = best.idx;
            bool accept = false;
            if (pending && best.any()) {
                const BestTwoLevels t = unpack(best);
                // :146-166  bestDist <= TH_HIGH, and not (bestLevel == bestLevel2 && bestDist > mfNNratio * bestDist2);  LastFrame (:2103): bestDist <= TH_HIGH
                accept = t.bestDist <= th_high && (LASTFRAME || !(t.bestLevel == t.bestLevel2 && (float)t.bestDist > __fmul_rn(nnratio, (float)t.bestDist2)));
            }
            // 2. claims that occupy
            const bool claims = accept && obs;
            if (claims) atomicMin(&s_claim[idx1], (unsigned)lane);
            ORBX_WAVE_SYNC();
            // 3. dirty: an earlier lane claims one of my free candidates
            bool dirty = false;
            if (pending) {
                for (int k = 0; k < cnt; k++) {
                    const int idx = entries[st + k].x;
                    if (s_claim[idx] < (unsigned)lane) { dirty = true; break; }
                }
            }
            const unsigned long long dmask = __ballot(dirty);
            const int first_dirty = dmask ? __ffsll(dmask) - 1 : 64;
            ORBX_WAVE_SYNC();
            if (claims) s_claim[idx1] = 0xFFu;                         // (every claimer of a slot restores it: the slot is 0xFF again for the next round)
            ORBX_WAVE_SYNC();
            // 4. commit the lanes before the first dirty one
            const bool commit = pending && lane < first_dirty;
            if (commit && accept) {
                atomicMax(&assigned[idx1], qi);
                if (obs) atomicOr(&s_occ[idx1 >> 5], 1u << (idx1 & 31));
                if (LASTFRAME && check_ori) {                          // angle(last) - angle(current) (:2118-2125)
                    const int bin = rot_bin(last_angle[qi], cur_kps[idx1].angle);
                    atomicAdd(&s_hist[bin & 31], 1);
                    events[qi] = idx1 | (bin << 16);
                }
            }
            nm += __popcll(__ballot(commit && accept));
            if (commit) pending = false;
            ORBX_WAVE_SYNC();
        }
    }
    if (LASTFRAME && check_ori) {
        ORBX_WAVE_SYNC();
        const ThreeMaxima top = three_maxima(s_hist);
        int taken_back = 0;
        for (int qi = lane; qi < M; qi += 64) {
            const int ev = events[qi];
            if (ev < 0) continue;
            if (!top.keeps(ev >> 16)) { assigned[ev & 0xFFFF] = -2; taken_back++; }
        }
        nm -= wave_sum(taken_back);
    }
    if (lane == 0) nmatches[b] = nm;
}

__global__ void __launch_bounds__(64) k_local_accept(const FrameMapRec* __restrict__ maps, int cap, const int* __restrict__ n_per_frame, const int* __restrict__ q_start,
                                                     const int* __restrict__ q_count, const int2* __restrict__ entries, const uint8_t* __restrict__ occupied0,
                                                     const uint8_t* __restrict__ has_obs, float nnratio, int th_high, int* __restrict__ assigned,
                                                     int* __restrict__ nmatches) {
    local_accept_body<false>(maps, cap, n_per_frame, q_start, q_count, entries, occupied0, has_obs, nnratio, th_high, assigned, nmatches, nullptr, nullptr, 0);
}
__global__ void __launch_bounds__(64) k_lastframe_accept(const FrameMapRec* __restrict__ maps, int cap, const int* __restrict__ n_per_frame, const int* __restrict__ q_start,
                                                         const int* __restrict__ q_count, const int2* __restrict__ entries, const uint8_t* __restrict__ occupied0,
                                                         const uint8_t* __restrict__ has_obs, int th_high, int* __restrict__ assigned, int* __restrict__ nmatches,
                                                         const float* __restrict__ last_angle, const KeyPointRec* __restrict__ cur_kps, int check_ori) {
    local_accept_body<true>(maps, cap, n_per_frame, q_start, q_count, entries, occupied0, has_obs, 0.0f, th_high, assigned, nmatches, last_angle, cur_kps, check_ori);
}

// ---- two-camera rig frames (Frame::Nleft != -1) in a batch ----
// Frame::isInFrustum with two cameras (src/Frame.cc:754-766 -> isInFrustumChecks :1592-1650, once per camera) and the window queries of both passes
// of SearchByProjection(Frame, MapPoints) for B rig frames.  Fb = [B][2]: camera 1 and camera 2 of frame b, both in rig_mode.  Camera 1's query is
// the one frustum_body writes (the search runs with the right-coordinate gate off: a rig frame has no mvuRight).  Camera 2's (src/ORBmatcher.cc:
// 170-176): the point is alive (in view of either camera, not far by camera 1's depth, not bad), in camera 2's view with a level; radius
// RadiusByViewingCos(mTrackViewCosR) WITHOUT th; levels [level - 1, level].  Frame b reads the set maps[b] names, its is_bad row at maps[b].flags, and
// every output of either camera sits at maps[b].offset (track: 5 x offset), as in k_frustum_batch.
// (the body, point i of a frame: every array is THAT frame's - M rows, track 5 M)
__device__ __forceinline__ void frustum_rig_body(const FrustumParams& F1, const FrustumParams& F2, int i, int M, const float* __restrict__ pos,
                                                 const float* __restrict__ normal, const float* __restrict__ min_dist, const float* __restrict__ max_dist,
                                                 const uint8_t* __restrict__ is_bad, uint8_t* in_view1, uint8_t* in_view2, float* track1, float* track2, int* level1,
                                                 int* level2, AreaQuery* __restrict__ q1, AreaQuery* __restrict__ q2) {
    const size_t Ms = (size_t)M;
    frustum_body(F1, i, M, pos, normal, min_dist, max_dist, is_bad, in_view1, track1, level1, q1);
    frustum_body(F2, i, M, pos, normal, min_dist, max_dist, is_bad, in_view2, track2, level2, nullptr);
    // (this thread's own stores, read back)
    const bool inl = in_view1[i] != 0, inr = in_view2[i] != 0;
    const int lvl = level2[i];
    AreaQuery q; q.x = 0; q.y = 0; q.r = 0; q.ur = 0; q.min_level = 0; q.max_level = 0; q.active = 0; q.gate = 0;
    const bool alive = (inl || inr) && !(F1.far_points && track1[3 * Ms + i] > F1.th_far) && !(is_bad && is_bad[i]);
    if (alive && inr && lvl >= 0 && lvl < F2.nlevels) {
        const float r = (double)track2[4 * Ms + i] > 0.998 ? 2.5f : 4.0f;
        q.x = track2[i]; q.y = track2[Ms + i]; q.r = __fmul_rn(r, pick(F2.scale_factors, lvl));
        q.min_level = lvl - 1; q.max_level = lvl; q.active = 1;
    }
    q2[i] = q;
}
__global__ void __launch_bounds__(256) k_frustum_rig(const FrustumParams* __restrict__ Fb, const FrameMapRec* __restrict__ maps, const uint8_t* __restrict__ is_bad,
                                                     uint8_t* in_view1, uint8_t* in_view2, float* track1, float* track2, int* level1, int* level2,
                                                     AreaQuery* __restrict__ q1, AreaQuery* __restrict__ q2, int* __restrict__ zero4) {
    const size_t b = blockIdx.y;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (zero4 && i < 4 && b == 0) zero4[i] = 0;
    const FrameMapRec T = maps[b];
    if (i >= T.M) return;
    const size_t o = (size_t)T.offset, ot = 5 * o;
    frustum_rig_body(Fb[2 * b], Fb[2 * b + 1], i, T.M, T.pos, T.normal, T.min_d, T.max_d, is_bad + T.flags, in_view1 + o, in_view2 + o, track1 + ot, track2 + ot, level1 + o,
                     level2 + o, q1 + o, q2 + o);
}

// The head of SearchByProjection(CurrentFrame, LastFrame) for B rig frames: camera 1 exactly as k_lastframe_queries; camera 2 (src/ORBmatcher.cc:
// 2089-2100) for every point whose camera-1 query exists: x3Dr = mTrl * x3Dc (Sophus' quaternion action), projected with CurrentFrame.mpCamera
// (camera 1's model - the reference's own choice), no depth or image test, the same radius and level window, no right-coordinate gate.
__global__ void __launch_bounds__(256) k_lastframe_queries_rig(const FrustumParams* __restrict__ Fb, int capL, const int* __restrict__ n_last,
                                                               const float* __restrict__ pos, const uint8_t* __restrict__ valid, const int* __restrict__ octave,
                                                               RigRelPose trl, AreaQuery* q1, AreaQuery* __restrict__ q2, int* __restrict__ zero4) {
    projection_queries_body<false>(Fb, capL, n_last, pos, valid, octave, nullptr, nullptr, q1, zero4);
    const size_t b = blockIdx.y;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= capL) return;
    const size_t o = b * (size_t)capL + i;
    const AreaQuery A = q1[o];                                     // (this thread's own store)
    AreaQuery q; q.x = 0; q.y = 0; q.r = 0; q.ur = 0; q.min_level = 0; q.max_level = 0; q.active = 0; q.gate = 0;
    if (A.active) {
        const FrustumParams& F = Fb[b];
        const float P0 = pos[3 * o], P1 = pos[3 * o + 1], P2 = pos[3 * o + 2];
        float pc[3];
        if (F.debug_flags & 16) se3_act_matrix_form(F.qcw, F.tcw, P0, P1, P2, pc);
        else se3_act(F.qcw, F.tcw, P0, P1, P2, pc);
        se3_act(trl.q, trl.t, pc[0], pc[1], pc[2], pc);
        const float x = pc[0], y = pc[1], z = pc[2];
        float u, v;
        if (F.kb8) { KB8Cam c; for (int k = 0; k < 8; k++) c.p[k] = F.cam[k]; const float pcc[3] = {x, y, z}; float uv[2]; kb8_project(c, pcc, uv); u = uv[0]; v = uv[1]; }
        else { u = __fadd_rn(__fdiv_rn(__fmul_rn(F.cam[0], x), z), F.cam[2]); v = __fadd_rn(__fdiv_rn(__fmul_rn(F.cam[1], y), z), F.cam[3]); }
        q.x = u; q.y = v; q.r = A.r; q.min_level = A.min_level; q.max_level = A.max_level; q.active = 1;
    }
    q2[o] = q;
}

// The accept loops of both searches for rig frames, one wave per frame, in the joint slot space of F.mvpMapPoints: camera 1's keypoint i at slot i,
// camera 2's keypoint j at slot Nleft + j.  The optimistic scheme of local_accept_body, per map point (lane) in point order:
//   camera-1 pass against the current occupancy; MapPoints form (src/ORBmatcher.cc:62-168): a ratio-test rejection ends the point (`continue`),
//   an accept writes the best slot AND its stereo partner Nleft + mvLeftToRightMatch[best] (partner writes ignore occupancy, as the reference's do);
//   camera-2 pass (:170-236) against the occupancy with this point's own camera-1 writes applied; an accept writes Nleft + best and
//   mvRightToLeftMatch[best].  LastFrame form (:2025-2152): best only, an empty camera-1 window ends the point, no partners, every accept is an
//   event of ONE rotation histogram over both cameras.
// Every write sets the slot's occupancy to the point's has_obs (F.mvpMapPoints[slot] = pMP: a partner write of a point without observations frees an
// occupied slot).  A lane claims the slots whose occupancy its writes change; it is dirty when an earlier lane of the round claims a candidate of
// either of its windows; lanes before the first dirty one commit.  The sequential last writer of a slot is the largest point index (atomicMax on
// assigned); among the lanes committing in one round, the largest lane writing a slot sets its occupancy.
// Frame b has maps[b].M points; its query rows (LastFrame form: and last_angle) start at maps[b].offset, its has_obs row at maps[b].flags.
// occupied0: [B][2 cap] bytes in the joint slot layout or NULL; has_obs: NULL = all observed; l2r / r2l: [B][cap];
// assigned: [B][2 cap]; nmatches: [B].  dynamic LDS: claim word per slot (2 cap words) | occupancy byte per slot (2 cap, 16-byte multiple) | LastFrame:
// two events per query (2 M words, slot * 32 + bin).
template <bool LASTFRAME>
__device__ __forceinline__ void rig_accept_body(const FrameMapRec* __restrict__ maps, int cap, const int* __restrict__ n1, const int* __restrict__ n2, const int* __restrict__ qs1,
                                                const int* __restrict__ qc1, const int* __restrict__ qs2, const int* __restrict__ qc2,
                                                const int2* __restrict__ entries, const uint8_t* __restrict__ occupied0, const uint8_t* __restrict__ has_obs,
                                                const int* __restrict__ l2r, const int* __restrict__ r2l, float nnratio, int th_high, int* __restrict__ assigned,
                                                int* __restrict__ nmatches, const float* __restrict__ last_angle, const KeyPointRec* __restrict__ kps1,
                                                const KeyPointRec* __restrict__ kps2, int check_ori) {
    ORBX_DYN_SMEM(smem);
    const int S = 2 * cap;
    unsigned* s_claim = (unsigned*)smem;
    uint8_t* s_occ = smem + 4 * (size_t)S;                        // one byte per slot: the last writer of a slot stores its has_obs, set or clear
    int* events = LASTFRAME ? (int*)(s_occ + (((size_t)S + 15) & ~(size_t)15)) : nullptr;
    __shared__ int s_hist[32];
    const int lane = lane_id();
    const size_t b = blockIdx.x;
    const int NL = n1[b], NR = n2[b], NS = NL + NR;
    const int M = maps[b].M;
    const size_t qo = (size_t)maps[b].offset;
    qs1 += qo; qc1 += qo; qs2 += qo; qc2 += qo; assigned += b * (size_t)S;
    if (has_obs) has_obs += maps[b].flags;
    if (LASTFRAME) {
        last_angle += qo; kps1 += b * (size_t)cap; kps2 += b * (size_t)cap;
        if (lane < 32) s_hist[lane] = 0;
    } else { l2r += b * (size_t)cap; r2l += b * (size_t)cap; }
    for (int i = lane; i < S; i += 64) {
        assigned[i] = -1; s_claim[i] = 0xFFu;
        s_occ[i] = (occupied0 && i < NS && occupied0[b * (size_t)S + i]) ? 1 : 0;
    }
    ORBX_WAVE_SYNC();
    int nm = 0;
    for (int i0 = 0; i0 < M; i0 += 64) {
        const int qi = i0 + lane;
        const int c1 = qi < M ? qc1[qi] : 0, st1 = qi < M ? qs1[qi] : 0, c2 = qi < M ? qc2[qi] : 0, st2 = qi < M ? qs2[qi] : 0;
        const bool obs = qi < M && (!has_obs || has_obs[qi]);
        bool pending = LASTFRAME ? c1 > 0 : (c1 > 0 || c2 > 0);
        if (LASTFRAME && qi < M) { events[2 * qi] = -1; events[2 * qi + 1] = -1; }
        while (__ballot(pending) != 0ull) {
            // 1. this point's decision against the current occupancy: the slots it writes (camera-1 best, its partner, camera-2 best, its partner)
            int w0 = -1, w1 = -1, w2 = -1, w3 = -1;
            if (pending) {
                bool end = false;
                const BestTwo best1 = best_two_scan(entries, st1, c1, [&](int i) { return s_occ[i] != 0; });
                const BestTwoLevels t1 = unpack(best1);
                if (best1.any() && t1.bestDist <= th_high) {
                    if (!LASTFRAME && t1.bestLevel == t1.bestLevel2 && (float)t1.bestDist > __fmul_rn(nnratio, (float)t1.bestDist2)) end = true;
                    else {
                        w0 = best1.idx;
                        if (!LASTFRAME) { const int j = l2r[best1.idx]; if ((unsigned)j < (unsigned)NR) w1 = NL + j; }
                    }
                }
                if (!end && c2 > 0) {
                    // (this point's own partner write counts as the occupancy it leaves)
                    const BestTwo best2 = best_two_scan(entries, st2, c2, [&](int i) { const int s = NL + i; return s == w1 ? obs : s_occ[s] != 0; });
                    const BestTwoLevels t2 = unpack(best2);
                    if (best2.any() && t2.bestDist <= th_high) {
                        if (LASTFRAME || !(t2.bestLevel == t2.bestLevel2 && (float)t2.bestDist > __fmul_rn(nnratio, (float)t2.bestDist2))) {
                            w2 = NL + best2.idx;
                            if (!LASTFRAME) { const int j = r2l[best2.idx]; if ((unsigned)j < (unsigned)NL) w3 = j; }
                        }
                    }
                }
            }
            const int ws[4] = {w0, w1, w2, w3};
            // 2. claims: the slots whose occupancy this point's writes change
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int s = ws[k];
                if (s >= 0 && (s_occ[s] != 0) != obs) atomicMin(&s_claim[s], (unsigned)lane);
            }
            ORBX_WAVE_SYNC();
            // 3. dirty: an earlier lane claims a candidate of either window
            bool dirty = false;
            if (pending) {
                for (int k = 0; k < c1 && !dirty; k++) if (s_claim[entries[st1 + k].x] < (unsigned)lane) dirty = true;
                for (int k = 0; k < c2 && !dirty; k++) if (s_claim[NL + entries[st2 + k].x] < (unsigned)lane) dirty = true;
            }
            const unsigned long long dmask = __ballot(dirty);
            const int first_dirty = dmask ? __ffsll(dmask) - 1 : 64;
            ORBX_WAVE_SYNC();
#pragma unroll
            for (int k = 0; k < 4; k++) if (ws[k] >= 0) s_claim[ws[k]] = 0xFFu;
            ORBX_WAVE_SYNC();
            // 4. commit the lanes before the first dirty one; the largest committing lane that writes a slot decides its occupancy
            const bool commit = pending && lane < first_dirty;
            if (commit) {
#pragma unroll
                for (int k = 0; k < 4; k++) if (ws[k] >= 0) { atomicMax(&assigned[ws[k]], qi); atomicMin(&s_claim[ws[k]], (unsigned)(63 - lane)); }
            }
            ORBX_WAVE_SYNC();
            if (commit) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int s = ws[k];
                    if (s >= 0 && s_claim[s] == (unsigned)(63 - lane)) s_occ[s] = obs ? 1 : 0;
                }
            }
            ORBX_WAVE_SYNC();
            if (commit) {
#pragma unroll
                for (int k = 0; k < 4; k++) if (ws[k] >= 0) s_claim[ws[k]] = 0xFFu;
                if (LASTFRAME && check_ori) {                          // angle(last) - angle(current) (:2118-2125)
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        const int s = c == 0 ? w0 : w2;
                        if (s < 0) continue;
                        const int bin = rot_bin(last_angle[qi], c == 0 ? kps1[s].angle : kps2[s - NL].angle);
                        atomicAdd(&s_hist[bin & 31], 1);
                        events[2 * qi + c] = s * 32 + (bin & 31);
                    }
                }
            }
            nm += wave_sum(commit ? (int)(w0 >= 0) + (int)(w1 >= 0) + (int)(w2 >= 0) + (int)(w3 >= 0) : 0);
            if (commit) pending = false;
            ORBX_WAVE_SYNC();
        }
    }
    if (LASTFRAME && check_ori) {
        ORBX_WAVE_SYNC();
        const ThreeMaxima top = three_maxima(s_hist);
        int taken_back = 0;
        for (int e = lane; e < 2 * M; e += 64) {
            const int ev = events[e];
            if (ev < 0) continue;
            if (!top.keeps(ev & 31)) { assigned[ev >> 5] = -2; taken_back++; }
        }
        nm -= wave_sum(taken_back);
    }
    if (lane == 0) nmatches[b] = nm;
}

__global__ void __launch_bounds__(64) k_rig_local_accept(const FrameMapRec* __restrict__ maps, int cap, const int* __restrict__ n1, const int* __restrict__ n2,
                                                         const int* __restrict__ qs1, const int* __restrict__ qc1, const int* __restrict__ qs2,
                                                         const int* __restrict__ qc2, const int2* __restrict__ entries, const uint8_t* __restrict__ occupied0,
                                                         const uint8_t* __restrict__ has_obs, const int* __restrict__ l2r, const int* __restrict__ r2l, float nnratio,
                                                         int th_high, int* __restrict__ assigned, int* __restrict__ nmatches) {
    rig_accept_body<false>(maps, cap, n1, n2, qs1, qc1, qs2, qc2, entries, occupied0, has_obs, l2r, r2l, nnratio, th_high, assigned, nmatches, nullptr, nullptr, nullptr, 0);
}
__global__ void __launch_bounds__(64) k_rig_lastframe_accept(const FrameMapRec* __restrict__ maps, int cap, const int* __restrict__ n1, const int* __restrict__ n2,
                                                             const int* __restrict__ qs1, const int* __restrict__ qc1, const int* __restrict__ qs2,
                                                             const int* __restrict__ qc2, const int2* __restrict__ entries, const uint8_t* __restrict__ occupied0,
                                                             const uint8_t* __restrict__ has_obs, int th_high, int* __restrict__ assigned, int* __restrict__ nmatches,
                                                             const float* __restrict__ last_angle, const KeyPointRec* __restrict__ kps1,
                                                             const KeyPointRec* __restrict__ kps2, int check_ori) {
    rig_accept_body<true>(maps, cap, n1, n2, qs1, qc1, qs2, qc2, entries, occupied0, has_obs, nullptr, nullptr, 0.0f, th_high, assigned, nmatches, last_angle, kps1, kps2, check_ori);
}

// Frame::ComputeStereoFromRGBD (src/Frame.cc:1361-1391) for B frames: mvDepth[i] = imDepth.at<float>(v, u) at the (distorted) keypoint, truncated
// to integers like cv::Mat::at(int, int) with float arguments, and mvuRight[i] = kpU.pt.x - mbf / d where d > 0, else both -1.  keys_un == NULL:
// no distortion (mvKeysUn = mvKeys).  depth image b at depth + b * image_stride (floats), rows `stride` floats apart.
__global__ void __launch_bounds__(256) k_stereo_from_depth(const KeyPointRec* __restrict__ kps, const KeyPointRec* __restrict__ kps_un, const int* __restrict__ n_per_frame,
                                                           int cap, const float* __restrict__ depth, int stride, size_t image_stride, int w, int h, float mbf,
                                                           float* __restrict__ u_right, float* __restrict__ depth_out, int* __restrict__ n_valid) {
    const size_t b = blockIdx.y;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= cap) return;
    float ur = -1.0f, d_out = -1.0f;
    if (i < n_per_frame[b]) {
        const KeyPointRec kp = kps[b * (size_t)cap + i];
        const int u = (int)kp.x, v = (int)kp.y;
        if (u >= 0 && u < w && v >= 0 && v < h) {
            const float d = depth[b * image_stride + (size_t)v * stride + u];
            if (d > 0) {
                const float xu = kps_un ? kps_un[b * (size_t)cap + i].x : kp.x;
                d_out = d; ur = __fsub_rn(xu, __fdiv_rn(mbf, d));
                atomicAdd(&n_valid[b], 1);
            }
        }
    }
    u_right[b * (size_t)cap + i] = ur; depth_out[b * (size_t)cap + i] = d_out;
}

// One wave per work item (an unmatched feature idx1 of KF1 and the feature list of a neighbour KF2 in the same node; the arrays of
// all neighbours of a batch are concatenated, item.out_off = neighbour).  best2[item] = chosen (global) idx2 or -1.   src/ORBmatcher.cc:1117-1254
// The best candidate for feature idx1 of KF1 (record k1, descriptor a0..a3) among cnt2 features of KF2 listed in feat2 (one vocabulary
// node): src/ORBmatcher.cc:1117-1254.  Returns the chosen entry of feat2 or -1.  One wave; every lane gets the result.
template <bool KB8>
__device__ __forceinline__ int bow_search_core(int idx1, const KeyPointRec k1, bool stereo1, unsigned long long a0, unsigned long long a1,
                                               unsigned long long a2, unsigned long long a3, const BowParams& P,
                                               const KeyPointRec* __restrict__ kps2, const unsigned long long* __restrict__ desc2,
                                               const float* __restrict__ ur2, const uint8_t* __restrict__ has_mp2,
                                               const int* __restrict__ feat2, int cnt2) {
    const int lane = lane_id();
    // epipolar line of kp1 in image 2 (Pinhole::epipolarConstrain, src/CameraModels/Pinhole.cpp:186-217)
    const float la = __fadd_rn(__fadd_rn(__fmul_rn(k1.x, P.F12[0]), __fmul_rn(k1.y, P.F12[3])), P.F12[6]);
    const float lb = __fadd_rn(__fadd_rn(__fmul_rn(k1.x, P.F12[1]), __fmul_rn(k1.y, P.F12[4])), P.F12[7]);
    const float lc = __fadd_rn(__fadd_rn(__fmul_rn(k1.x, P.F12[2]), __fmul_rn(k1.y, P.F12[5])), P.F12[8]);
    const float den = __fadd_rn(__fmul_rn(la, la), __fmul_rn(lb, lb));
    // Kannala-Brandt cameras: which camera of a rig the feature belongs to (:1136-1141), its ray (unprojected once per feature)
    const bool rig = KB8 && P.nleft1 >= 0 && P.nleft2 >= 0;                          // pKF1->mpCamera2 && pKF2->mpCamera2 (:1203)
    const int right1 = (KB8 && P.nleft1 >= 0 && idx1 >= P.nleft1) ? 1 : 0;
    KB8Cam c1; float ray1[3] = {0.f, 0.f, 1.f};
    if (KB8) {
#pragma unroll
        for (int i = 0; i < 8; i++) c1.p[i] = P.cam1[rig ? right1 : 0][i];
        kb8_unproject(c1, k1.x, k1.y, ray1);
    }
    unsigned best = 0xFFFFFFFFu;   // dist << 16 | (0xFFFF - position): the LAST candidate with the smallest distance wins (:1178 '>' test)
    for (int j = lane; j < cnt2; j += 64) {
        const int idx2 = feat2[j];
        if (has_mp2[idx2]) continue;
        const bool stereo2 = ur2[idx2] >= 0;
        if (P.only_stereo && !stereo2) continue;
        const unsigned long long* db = desc2 + 4 * (size_t)idx2;
        const int dist = __popcll(a0 ^ db[0]) + __popcll(a1 ^ db[1]) + __popcll(a2 ^ db[2]) + __popcll(a3 ^ db[3]);
        if (dist > P.th_low) continue;
        const KeyPointRec k2 = kps2[idx2];
        if (!stereo1 && !stereo2 && !(KB8 && P.nleft1 >= 0)) {                       // ... && !pKF1->mpCamera2 (:1189)
            const float dex = __fsub_rn(P.ep[0], k2.x), dey = __fsub_rn(P.ep[1], k2.y);
            if (__fadd_rn(__fmul_rn(dex, dex), __fmul_rn(dey, dey)) < __fmul_rn(100.f, P.scale2[k2.octave])) continue;
        }
        if (KB8) {
            if (!P.coarse) {
                const int right2 = (P.nleft2 >= 0 && idx2 >= P.nleft2) ? 1 : 0;
                const int sel = rig ? right1 * 2 + right2 : 0;
                KB8Cam c2; float ray2[3], p3D[3];
#pragma unroll
                for (int i = 0; i < 8; i++) c2.p[i] = P.cam2[rig ? right2 : 0][i];
                kb8_unproject(c2, k2.x, k2.y, ray2);
                const float z = kb8_triangulate_matches(c1, c2, ray1, ray2, k1.x, k1.y, k2.x, k2.y, P.R[sel], P.t[sel], P.sigma2_1[k1.octave], P.sigma2_2[k2.octave], p3D);
                if (!(z > 0.0001f)) continue;                                            // KannalaBrandt8::epipolarConstrain (:322-328)
            }
        } else if (!P.coarse) {
            const float num = __fadd_rn(__fadd_rn(__fmul_rn(la, k2.x), __fmul_rn(lb, k2.y)), lc);
            if (den == 0) continue;
            const float dsqr = __fdiv_rn(__fmul_rn(num, num), den);
            if (!((double)dsqr < 3.84 * (double)P.sigma2_2[k2.octave])) continue;
        }
        const unsigned key = ((unsigned)dist << 16) | (unsigned)(0xFFFF - j);
        best = key < best ? key : best;
    }
    best = wave_min_u32(best);
    return best == 0xFFFFFFFFu ? -1 : feat2[0xFFFF - (int)(best & 0xFFFF)];
}

// One wave per work item (an unmatched feature idx1 of KF1 and the feature list of a neighbour KF2 in the same node; the arrays of
// all neighbours of a batch are concatenated, item.out_off = neighbour).  best2[item] = chosen (global) idx2 or -1.
template <bool KB8>
__device__ __forceinline__ void bow_search_body(const BowItem* __restrict__ items, int nitems,
                                                    const KeyPointRec* __restrict__ kps1, const unsigned long long* __restrict__ desc1,
                                                    const float* __restrict__ ur1,
                                                    const KeyPointRec* __restrict__ kps2, const unsigned long long* __restrict__ desc2,
                                                    const float* __restrict__ ur2, const uint8_t* __restrict__ has_mp2,
                                                    const int* __restrict__ feat2, const BowParams* __restrict__ Ps, int* __restrict__ best2) {
    const int lane = lane_id();
    const int it = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (it >= nitems) return;
    const BowItem I = items[it];
    const BowParams& P = Ps[I.out_off];            // the neighbour key frame this item belongs to (wave-uniform)
    const unsigned long long* da = desc1 + 4 * (size_t)I.idx1;
    const int r = bow_search_core<KB8>(I.idx1, kps1[I.idx1], ur1[I.idx1] >= 0, da[0], da[1], da[2], da[3], P, kps2, desc2, ur2, has_mp2, feat2 + I.start2, I.cnt2);
    if (lane == 0) best2[it] = r;
}

// Position of `id` in the ascending list ids[0, n), or -1: two 64-way probes by the whole wave instead of a dependent binary search.
__device__ __forceinline__ int wave_find_node(const uint32_t* __restrict__ ids, int n, uint32_t id) {
    const int lane = lane_id();
    int lo = 0, len = n;
    while (len > 64) {
        const int stride = (len + 63) >> 6;
        const int pos = lo + lane * stride;
        const unsigned long long le = __ballot(pos < lo + len && ids[pos] <= id);
        if (le == 0ull) return -1;
        const int seg = 63 - __clzll((long long)le);          // last probe <= id
        const int nlo = lo + seg * stride;
        len = imin(stride, lo + len - nlo); lo = nlo;
    }
    const unsigned long long eq = __ballot(lane < len && ids[lo + lane] == id);
    return eq ? lo + (__ffsll((long long)eq) - 1) : -1;
}

// ORBmatcher::SearchForTriangulation over device-resident key frames: one wave per (feature idx1 of KF1, neighbour j), no work list - the
// wave finds the neighbour's feature list of idx1's vocabulary node itself.  best[j * N1 + idx1] = index in neighbour j or -1.
// grid (ceil(N1 / 4), n2).  flags: call-time map point flags, KF1's at offset 0, neighbour j's at nb[j].mp2_off.
template <bool KB8>
__device__ __forceinline__ void sft_resident_body(const ResidentKF& k1, const uint8_t* __restrict__ flags, const SftNeighbour* __restrict__ nb, int* __restrict__ best) {
    const int lane = lane_id();
    const int idx1 = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), j = (int)blockIdx.y;
    if (idx1 >= k1.N) return;
    int r = -1;
    const SftNeighbour& S = nb[j];
    const int a = k1.node_of_feat[idx1];
    const bool stereo1 = k1.ur[idx1] >= 0;
    if (a >= 0 && !flags[idx1] && !(S.P.only_stereo && !stereo1)) {
        const int b = wave_find_node(S.k2.node_id, S.k2.fv_nodes, k1.node_id[a]);
        if (b >= 0) {
            const int s2 = S.k2.fv_start[b], c2 = S.k2.fv_start[b + 1] - s2;
            const unsigned long long* da = k1.desc + 4 * (size_t)idx1;
            r = bow_search_core<KB8>(idx1, k1.kps[idx1], stereo1, da[0], da[1], da[2], da[3], S.P, S.k2.kps, S.k2.desc, S.k2.ur, flags + S.mp2_off,
                                     S.k2.fv_feat + s2, c2);
        }
    }
    if (lane == 0) best[(size_t)j * k1.N + idx1] = r;
}
__global__ void __launch_bounds__(256) k_sft_resident(ResidentKF k1, const uint8_t* __restrict__ flags, const SftNeighbour* __restrict__ nb,
                                                      int* __restrict__ best) {
    sft_resident_body<false>(k1, flags, nb, best);
}
// Kannala-Brandt cameras (its own kernel for the same reason as k_bow_search_kb8)
__global__ void __launch_bounds__(256) k_sft_resident_kb8(ResidentKF k1, const uint8_t* __restrict__ flags, const SftNeighbour* __restrict__ nb,
                                                          int* __restrict__ best) {
    sft_resident_body<true>(k1, flags, nb, best);
}

// ORBmatcher::SearchByBoW (src/ORBmatcher.cc:259-493 and :892-1043, non-fisheye) over device-resident key frames, the sequential accept
// loop included: a target taken by an earlier feature is skipped (:331, :948), and since a feature of K2 belongs to exactly one vocabulary
// node, that dependence never leaves a node - one wave per (node of K1, pair) walks the node's K1 features in order.
// A lane owns the candidates (positions in K2's list of the node) lane, lane + 64, ..; bit r of `taken` = position lane + 64 r is taken.
// RIG: K2 is a rig frame (F.Nleft != -1, :343-372 and :414-446): its features below nleft are camera 1's, the others camera 2's; camera 1 keeps best
// and second best, camera 2 only its best (its ratio test is `|| true`, :419) and is considered only when camera 1's best passed TH_LOW (:384).
// out: K2 index by K1 feature (out[idx1]), or for RIG the K1 feature by K2 index (out[idx2]) - every K2 feature is taken at most once.
template <bool RIG>
__device__ __forceinline__ void bow_match_node(const BowPairResident& B, int a, const uint8_t* __restrict__ flags, float nnratio, int th_low,
                                               int th_inclusive, int nleft, int* __restrict__ out, int* __restrict__ status) {
    const int lane = lane_id();
    if (a >= B.k1.fv_nodes || B.mp1_off < 0) return;
    const int b = wave_find_node(B.k2.node_id, B.k2_nodes_dev ? *B.k2_nodes_dev : B.k2.fv_nodes, B.k1.node_id[a]);
    if (b < 0) return;
    const int s2 = B.k2.fv_start[b], c2 = B.k2.fv_start[b + 1] - s2;
    if (c2 > 2048) { if (lane == 0) atomicOr(status, 4); return; }
    const uint8_t* mp1 = flags + B.mp1_off;
    const uint8_t* el2 = B.elig2_off >= 0 ? flags + B.elig2_off : nullptr;
    // this lane's candidates: index in K2 and eligibility, fetched once
    unsigned taken = 0;
    for (int k = B.k1.fv_start[a]; k < B.k1.fv_start[a + 1]; k++) {
        const int idx1 = B.k1.fv_feat[k];
        if (!mp1[idx1]) continue;                                                      // !pMP || pMP->isBad()
        const unsigned long long* da = B.k1.desc + 4 * (size_t)idx1;
        const unsigned long long a0 = da[0], a1 = da[1], a2 = da[2], a3 = da[3];
        unsigned k1key = (256u << 16) | 0xFFFFu, k2key = k1key, r1key = k1key;        // this lane's two smallest (distance << 16 | position); camera 2's smallest
        for (int j = lane, r = 0; j < c2; j += 64, r++) {
            if ((taken >> r) & 1u) continue;
            const int idx2 = B.k2.fv_feat[s2 + j];
            if (el2 && !el2[idx2]) continue;
            const unsigned long long* db = B.k2.desc + 4 * (size_t)idx2;
            const unsigned d = (unsigned)(__popcll(a0 ^ db[0]) + __popcll(a1 ^ db[1]) + __popcll(a2 ^ db[2]) + __popcll(a3 ^ db[3]));
            const unsigned key = (d << 16) | (unsigned)j;
            if (!RIG || idx2 < nleft) { if (key < k1key) { k2key = k1key; k1key = key; } else if (key < k2key) k2key = key; }
            else if (key < r1key) r1key = key;
        }
        // sequential rule: bestDist1 = smallest distance (first position that attains it), bestDist2 = second smallest of the multiset
        const unsigned m1 = wave_min_u32(k1key);
        const unsigned m2 = wave_min_u32(k1key == m1 ? k2key : k1key);
        const int bestDist1 = (int)(m1 >> 16), bestDist2 = (int)(m2 >> 16);
        const bool pass = th_inclusive ? bestDist1 <= th_low : bestDist1 < th_low;
        if (pass && (float)bestDist1 < __fmul_rn(nnratio, (float)bestDist2)) {
            const int j1 = (int)(m1 & 0xFFFFu);
            if (lane == (j1 & 63)) {
                taken |= 1u << (j1 >> 6);
                if (RIG) out[B.k2.fv_feat[s2 + j1]] = idx1; else out[idx1] = B.k2.fv_feat[s2 + j1];
            }
        }
        if (RIG && pass) {                                                             // uniform: m1 is the wave's
            const unsigned mr = wave_min_u32(r1key);
            if ((int)(mr >> 16) <= th_low) {
                const int jr = (int)(mr & 0xFFFFu);
                if (lane == (jr & 63)) { taken |= 1u << (jr >> 6); out[B.k2.fv_feat[s2 + jr]] = idx1; }
            }
        }
    }
}

// m12[p * N1cap + idx1] = matched index in K2 (pre-set to -1).  Nodes with more than 2048 features in K2 set status bit 2.
// grid (ceil(max fv_nodes / 4), n)
__global__ void __launch_bounds__(256) k_bow_match_resident(const BowPairResident* __restrict__ pairs, const uint8_t* __restrict__ flags,
                                                            float nnratio, int th_low, int th_inclusive, int* __restrict__ m12, int N1cap,
                                                            int* __restrict__ status) {
    const int a = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), p = (int)blockIdx.y;
    bow_match_node<false>(pairs[p], a, flags, nnratio, th_low, th_inclusive, 0, m12 + (size_t)p * N1cap, status);
}

// SearchByBoW(pKF, F) with a rig frame F (orbm_search_by_bow_rig_batch): assigned[p * S + j] = key-frame feature whose map point goes to
// F.mvpMapPoints[j] (pre-set to -1), j < Nleft + Nright.  TH_LOW inclusive (:378).  grid (ceil(max fv_nodes of the key frames / 4), pairs)
__global__ void __launch_bounds__(256) k_bow_match_rig(const BowPairRig* __restrict__ pairs, const uint8_t* __restrict__ flags, float nnratio, int th_low,
                                                       int* __restrict__ assigned, int S, int* __restrict__ status) {
    const int a = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), p = (int)blockIdx.y;
    const BowPairRig& R = pairs[p];
    bow_match_node<true>(R.m, a, flags, nnratio, th_low, 1, *R.nleft, assigned + (size_t)p * S, status);
}

// The rotation-consistency pruning behind SearchByBoW (src/ORBmatcher.cc:396-412 fill, :457-479 prune; ComputeThreeMaxima :2335-2377) on the device, one
// wave per pair: histogram of round((angle1 - angle2 [+ 360]) / 30) over the matches, entries outside the three strongest bins (the second / third
// only while they hold at least 10 % of the first) are reset to -1; returns the matches left (on every lane).  m [n]: one pair's results, bin_of(i, m[i]).
template <typename BinOf>
__device__ __forceinline__ int bow_prune_body(int* __restrict__ m, int n, int check_ori, int* s_hist, const BinOf& bin_of) {
    const int lane = lane_id();
    if (lane < 32) s_hist[lane] = 0;
    ORBX_WAVE_SYNC();
    int nm = 0;
    for (int i = lane; i < n; i += 64) {
        const int j = m[i];
        if (j < 0) continue;
        nm++;
        if (check_ori) atomicAdd(&s_hist[bin_of(i, j) & 31], 1);
    }
    ORBX_WAVE_SYNC();
    if (check_ori) {
        const ThreeMaxima top = three_maxima(s_hist);
        for (int i = lane; i < n; i += 64) {
            const int j = m[i];
            if (j < 0) continue;
            if (!top.keeps(bin_of(i, j))) { m[i] = -1; nm--; }
        }
    }
    return wave_sum(nm);
}

// m12 as written by k_bow_match_resident; nmatches[p] = matches left
__global__ void __launch_bounds__(64) k_bow_rotation_prune(const BowPairResident* __restrict__ pairs, int* __restrict__ m12, int N1cap, int check_ori,
                                                           int* __restrict__ nmatches) {
    __shared__ int s_hist[32];
    const int p = (int)blockIdx.x;
    const BowPairResident& B = pairs[p];
    const int nm = bow_prune_body(m12 + (size_t)p * N1cap, B.k1.N, check_ori, s_hist,
                                  [&](int i, int j) { return rot_bin(B.k1.kps[i].angle, B.k2.kps[j].angle); });
    if (lane_id() == 0) nmatches[p] = nm;
}

// the same over k_bow_match_rig's frame-indexed rows: one histogram for both cameras; the key frame's keypoint minus the frame's (mvKeys below
// Nleft, mvKeysRight above, :391-395 and :425-429); nmatches[p] = matches left, as the reference counts them (each match enters the histogram once)
__global__ void __launch_bounds__(64) k_bow_rotation_prune_rig(const BowPairRig* __restrict__ pairs, int* __restrict__ assigned, int S, int check_ori,
                                                               int* __restrict__ nmatches) {
    __shared__ int s_hist[32];
    const int p = (int)blockIdx.x;
    const BowPairRig& R = pairs[p];
    const int nleft = *R.nleft;
    const int nm = bow_prune_body(assigned + (size_t)p * S, S, check_ori, s_hist, [&](int j, int i) {
        return rot_bin(R.m.k1.kps[i].angle, j < nleft ? R.m.k2.kps[j].angle : R.kps_r[j - nleft].angle);
    });
    if (lane_id() == 0) nmatches[p] = nm;
}

__global__ void __launch_bounds__(256) k_bow_search(const BowItem* __restrict__ items, int nitems, const KeyPointRec* __restrict__ kps1,
                                                    const unsigned long long* __restrict__ desc1, const float* __restrict__ ur1,
                                                    const KeyPointRec* __restrict__ kps2, const unsigned long long* __restrict__ desc2,
                                                    const float* __restrict__ ur2, const uint8_t* __restrict__ has_mp2,
                                                    const int* __restrict__ feat2, const BowParams* __restrict__ Ps, int* __restrict__ best2) {
    bow_search_body<false>(items, nitems, kps1, desc1, ur1, kps2, desc2, ur2, has_mp2, feat2, Ps, best2);
}
// the same with Kannala-Brandt cameras (the triangulation test needs ~200 registers: its own kernel keeps the pinhole one slim)
__global__ void __launch_bounds__(256) k_bow_search_kb8(const BowItem* __restrict__ items, int nitems, const KeyPointRec* __restrict__ kps1,
                                                        const unsigned long long* __restrict__ desc1, const float* __restrict__ ur1,
                                                        const KeyPointRec* __restrict__ kps2, const unsigned long long* __restrict__ desc2,
                                                        const float* __restrict__ ur2, const uint8_t* __restrict__ has_mp2,
                                                        const int* __restrict__ feat2, const BowParams* __restrict__ Ps, int* __restrict__ best2) {
    bow_search_body<true>(items, nitems, kps1, desc1, ur1, kps2, desc2, ur2, has_mp2, feat2, Ps, best2);
}

// All distances of one unmatched feature idx1 to the features of the other key frame / frame in the same vocabulary node, in the
// node's order, for the sequential accept loops of ORBmatcher::SearchByBoW (src/ORBmatcher.cc:259-493 and :892-1043), which skip
// targets taken by earlier features.  out[item.out_off + j] = Hamming distance, or -1 when the j-th target is not eligible.
__global__ void __launch_bounds__(256) k_bow_dists(const BowItem* __restrict__ items, int nitems,
                                                   const unsigned long long* __restrict__ desc1, const unsigned long long* __restrict__ desc2,
                                                   const uint8_t* __restrict__ eligible2, const int* __restrict__ feat2, int* __restrict__ out) {
    const int lane = lane_id();
    const int it = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (it >= nitems) return;
    const BowItem I = items[it];
    const unsigned long long* da = desc1 + 4 * (size_t)I.idx1;
    const unsigned long long a0 = da[0], a1 = da[1], a2 = da[2], a3 = da[3];
    for (int j = lane; j < I.cnt2; j += 64) {
        const int idx2 = feat2[I.start2 + j];
        int d = -1;
        if (eligible2[idx2]) {
            const unsigned long long* db = desc2 + 4 * (size_t)idx2;
            d = __popcll(a0 ^ db[0]) + __popcll(a1 ^ db[1]) + __popcll(a2 ^ db[2]) + __popcll(a3 ^ db[3]);
        }
        out[I.out_off + j] = d;
    }
}

// ---- the resident map (orbm_map): the store of map-point fields by slot, and Tracking::UpdateLocalPoints (src/Tracking.cc:4088-4120) built from it ----
// A map point is 64 bytes: the descriptor (4 words of 8 bytes) and 8 floats (position 3 | normal 3 | mfMinDistance | mfMaxDistance).  Scatter and gather
// give a point to 4 neighbouring threads: thread q moves descriptor word q and floats 2 q, 2 q + 1, so a wave writes 16 whole descriptors side by side.
__device__ __forceinline__ float map_float_load(const float* pos, const float* normal, const float* min_d, const float* max_d, size_t i, int e) {
    return e < 3 ? pos[3 * i + e] : e < 6 ? normal[3 * i + (e - 3)] : e == 6 ? min_d[i] : max_d[i];
}
__device__ __forceinline__ void map_float_store(float* pos, float* normal, float* min_d, float* max_d, size_t i, int e, float v) {
    if (e < 3) pos[3 * i + e] = v; else if (e < 6) normal[3 * i + (e - 3)] = v; else if (e == 6) min_d[i] = v; else max_d[i] = v;
}

// orbm_map_update / orbm_map_set_bad: record r of the staged block goes to slot slots[r] (distinct: the host refuses duplicates, so no two records meet).
// desc == nullptr: the flag alone, and only where the slot holds a point.  grid (ceil(4 n / 256)), 256 threads
__global__ void __launch_bounds__(256) k_map_scatter(int n, const int* __restrict__ slots, const unsigned long long* __restrict__ desc, const float* __restrict__ pos,
                                                     const float* __restrict__ normal, const float* __restrict__ min_d, const float* __restrict__ max_d,
                                                     const uint8_t* __restrict__ bad, MapStore S) {
    const int t = (int)(blockIdx.x * 256u + threadIdx.x), r = t >> 2, q = t & 3;
    if (r >= n) return;
    const size_t slot = (size_t)slots[r];
    const uint8_t st = (uint8_t)(kMapPresent | (bad[r] ? kMapBad : 0));
    if (!desc) {
        if (q == 0 && (S.state[slot] & kMapPresent)) S.state[slot] = st;
        return;
    }
    S.desc[4 * slot + q] = desc[4 * (size_t)r + q];
    for (int e = 2 * q; e < 2 * q + 2; e++) map_float_store(S.pos, S.normal, S.min_d, S.max_d, slot, e, map_float_load(pos, normal, min_d, max_d, (size_t)r, e));
    if (q == 0) S.state[slot] = st;
}

// The slots frame b already holds (SearchLocalPoints' first loop, src/Tracking.cc:3983-4003) are marked with this call's epoch: every writer of a word
// stores the same value, so duplicates need no atomic.  grid (ceil(longest list / 256), B), 256 threads
__global__ void __launch_bounds__(256) k_map_seen(const int* __restrict__ seen_start, const int* __restrict__ seen_slots, unsigned* __restrict__ seen_stamp, int nslots,
                                                  unsigned mark) {
    const int b = (int)blockIdx.y, i = seen_start[b] + (int)(blockIdx.x * 256u + threadIdx.x);
    if (i < seen_start[b + 1]) seen_stamp[(size_t)b * nslots + seen_slots[i]] = mark;
}

// the slot at entry i of a visited row, or -1 where UpdateLocalPoints passes on (:4101-4105: no map point, or a bad one; a slot never updated counts as bad)
__device__ __forceinline__ int map_visit(const MapSeg& G, int i, const int* __restrict__ kf_slots, int row_cap, const uint8_t* __restrict__ state) {
    const int slot = kf_slots[(size_t)G.row * row_cap + i];
    return slot >= 0 && state[slot] == kMapPresent ? slot : -1;
}

// First occurrence (mnTrackReferenceForFrame, :4103-4109): position p of a frame's walk offers top - p to the stamp of (frame, slot); the largest offer is
// the earliest position, whatever order the atomics arrive in.  top = base + (largest position count of the call): this call's offers lie in (base, top],
// everything an earlier call left is <= base, and the next call starts at base = top - nothing is cleared between calls.
// grid (visited rows, ceil(longest row / kMapChunk)), kMapChunk threads
__global__ void __launch_bounds__(kMapChunk) k_map_stamp(const MapSeg* __restrict__ segs, const int* __restrict__ kf_slots, int row_cap, const uint8_t* __restrict__ state,
                                                         unsigned* __restrict__ stamp, int nslots, unsigned top) {
    const MapSeg G = segs[blockIdx.x];
    const int i = (int)(blockIdx.y * (unsigned)kMapChunk + threadIdx.x);
    if (i >= G.n) return;
    const int slot = map_visit(G, i, kf_slots, row_cap, state);
    if (slot >= 0) atomicMax(&stamp[(size_t)G.set * nslots + slot], top - (unsigned)(G.pos0 + i));
}

// The positions that keep their point, in visiting order: a chunk's survivors are counted with wave ballots (chunk_off == nullptr: chunk_cnt[chunk] is all
// this pass writes); once k_map_scan has turned the counts into offsets, the same ballots rank each survivor inside its chunk and its slot goes to
// sets[frame].slots[offset + rank].  No counter is shared between chunks, so the order is the walk's.  Same grid as k_map_stamp
__global__ void __launch_bounds__(kMapChunk) k_map_compact(const MapSeg* __restrict__ segs, const int* __restrict__ kf_slots, int row_cap, const uint8_t* __restrict__ state,
                                                           const unsigned* __restrict__ stamp, int nslots, unsigned top, int* __restrict__ chunk_cnt,
                                                           const int* __restrict__ chunk_off, const MapSetRec* __restrict__ sets) {
    __shared__ int wave_cnt[kMapChunk / 64];
    const MapSeg G = segs[blockIdx.x];
    const int i = (int)(blockIdx.y * (unsigned)kMapChunk + threadIdx.x);
    if ((int)(blockIdx.y * (unsigned)kMapChunk) >= G.n) return;            // (the whole workgroup: the row is shorter than the longest one)
    const int slot = i < G.n ? map_visit(G, i, kf_slots, row_cap, state) : -1;
    const bool keep = slot >= 0 && stamp[(size_t)G.set * nslots + slot] == top - (unsigned)(G.pos0 + i);
    const unsigned long long bal = __ballot(keep);
    const int lane = lane_id(), wave = wave_id();
    if (lane == 0) wave_cnt[wave] = __popcll(bal);
    __syncthreads();
    const int chunk = G.chunk0 + (int)blockIdx.y;
    if (!chunk_off) {
        if (threadIdx.x == 0) { int c = 0; for (int w = 0; w < kMapChunk / 64; w++) c += wave_cnt[w]; chunk_cnt[chunk] = c; }
        return;
    }
    if (!keep) return;
    int at = chunk_off[chunk] + __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) at += wave_cnt[w];
    sets[G.set].slots[at] = slot;
}

// exclusive scan of a frame's chunk counts (its chunks are frame_chunk0[b] .. frame_chunk0[b + 1] - 1) and their sum, the size of its local map.
// grid (B), one wave: a frame has a few hundred chunks
__global__ void __launch_bounds__(64) k_map_scan(const int* __restrict__ frame_chunk0, const int* __restrict__ chunk_cnt, int* __restrict__ chunk_off, int* __restrict__ M_out) {
    const int b = (int)blockIdx.x, lane = lane_id(), c1 = frame_chunk0[b + 1];
    int run = 0;
    for (int c = frame_chunk0[b]; c < c1; c += 64) {
        const int i = c + lane, v = i < c1 ? chunk_cnt[i] : 0;
        int incl = v;
        for (int d = 1; d < 64; d <<= 1) { const int up = __shfl_up(incl, d); if (lane >= d) incl += up; }
        if (i < c1) chunk_off[i] = run + incl - v;
        run += __shfl(incl, 63);
    }
    if (lane == 0) M_out[b] = run;
}

// the fields of every point of the built sets, by slot, and its seen flag (seen_stamp == nullptr: an explicit list, nothing seen).
// grid (ceil(4 x largest set / 256), sets), 256 threads
__global__ void __launch_bounds__(256) k_map_gather(const MapSetRec* __restrict__ sets, MapStore S, const unsigned* __restrict__ seen_stamp, int nslots, unsigned base) {
    const MapSetRec R = sets[blockIdx.y];
    const int t = (int)(blockIdx.x * 256u + threadIdx.x), j = t >> 2, q = t & 3;
    if (j >= R.M) return;
    const size_t slot = (size_t)R.slots[j];
    R.desc[4 * (size_t)j + q] = S.desc[4 * slot + q];
    for (int e = 2 * q; e < 2 * q + 2; e++) map_float_store(R.pos, R.normal, R.min_d, R.max_d, (size_t)j, e, map_float_load(S.pos, S.normal, S.min_d, S.max_d, slot, e));
    if (q == 0) R.seen[j] = seen_stamp ? (uint8_t)(seen_stamp[(size_t)R.set * nslots + slot] > base) : (uint8_t)0;
}

// ---- the rows of a projection batch read from the map (orbm_search_by_projection_lastframe_batch_map / _keyframe_batch_map) ------------------------
// Writes what the host-fed calls upload - valid, position, descriptor and, in the key-frame form, mfMinDistance, mfMaxDistance and the key frame's keypoint
// angle - for row i of frame b, so the query, window-search and accept kernels read the same block either way.  The row's slot is slots[b][i] (last frame:
// LastFrame.mvpMapPoints as slots, rows == nullptr) or entry i of the key frame's row in the map (rows[b].slots).  The row is valid iff i < n[b], the slot is
// >= 0 and holds a point, the caller's flag excluded[b][i] (mvbOutlier / sAlreadyFound) is 0 and - key-frame form only, src/ORBmatcher.cc:2218-2220 against
// :1981-1983 - the point is not bad.  Rows that are not valid are written as zeros.  Four lanes per row as k_map_gather: lane q moves descriptor word q
// and two of the floats {x y | z min | max angle}, lane 3 the valid byte.  grid (ceil(4 cap / 256), B), 256 threads
__global__ void __launch_bounds__(256) k_map_rows_gather(MapStore S, int cap, const int* __restrict__ n, const int* __restrict__ slots, const MapRowRec* __restrict__ rows,
                                                         const uint8_t* __restrict__ excluded, uint8_t* __restrict__ valid, float* __restrict__ pos,
                                                         unsigned long long* __restrict__ desc, float* __restrict__ min_d, float* __restrict__ max_d,
                                                         float* __restrict__ angle) {
    const int t = (int)(blockIdx.x * 256u + threadIdx.x), i = t >> 2, q = t & 3;
    if (i >= cap) return;
    const size_t b = blockIdx.y, o = b * (size_t)cap + (size_t)i;
    const bool inside = i < n[b];
    int slot = -1;
    if (inside) slot = rows ? rows[b].slots[i] : slots[o];
    bool ok = false;
    if (slot >= 0) {
        const uint8_t st = S.state[slot];
        ok = (st & kMapPresent) && !(rows && (st & kMapBad)) && !excluded[o];
    }
    const size_t s = ok ? (size_t)slot : 0;
    desc[4 * o + q] = ok ? S.desc[4 * s + q] : 0ull;
    if (q == 0) { pos[3 * o] = ok ? S.pos[3 * s] : 0.0f; pos[3 * o + 1] = ok ? S.pos[3 * s + 1] : 0.0f; }
    else if (q == 1) { pos[3 * o + 2] = ok ? S.pos[3 * s + 2] : 0.0f; if (rows) min_d[o] = ok ? S.min_d[s] : 0.0f; }
    else if (q == 2) { if (rows) { max_d[o] = ok ? S.max_d[s] : 0.0f; angle[o] = inside ? rows[b].kps[i].angle : 0.0f; } }
    else valid[o] = (uint8_t)ok;
}

// The call-time flags of the searches that name key frames by their row in the map, one record per flag array of the call: flags[off + i] = entry i of the
// row is a slot that holds a point which is not bad (kRowHoldsGoodPoint: `!pMP || pMP->isBad()`, src/ORBmatcher.cc:306-312, :938-941, :959-965 - the BoW
// searches) or a slot that holds a point, bad or not (kRowHoldsPoint: src/ORBmatcher.cc:1123-1127, :1159-1163 test the pointer only - SearchForTriangulation).
// grid (ceil(longest row / 256), records), 256 threads
__global__ void __launch_bounds__(256) k_map_row_flags(const int* __restrict__ kf_slots, int row_cap, const uint8_t* __restrict__ state,
                                                       const MapRowFlagRec* __restrict__ recs, uint8_t* __restrict__ flags) {
    const MapRowFlagRec R = recs[blockIdx.y];
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= R.n) return;
    const int slot = kf_slots[(size_t)R.row * row_cap + i];
    flags[(size_t)R.off + i] = (uint8_t)(slot >= 0 && (R.rule == kRowHoldsPoint ? (state[slot] & kMapPresent) != 0 : state[slot] == kMapPresent));
}

// ---- a batched SearchLocalPoints on the map's own sets (orbm_search_local_points_batch_map / _rig_batch_map) --------------------------------------
// The call-time flags of frame b, where BatchMaps::stage_flags would have put the caller's: is_bad = the seen bytes of the frame's set, has_obs = 1, both
// at recs[b].off in their blocks.  The blocks start at 16-byte multiples, so both destinations share their low address bits; off is a prefix sum of
// arbitrary M_b and aligned to nothing.  The destination is cut into up to 3 head bytes, whole dwords and up to 3 tail bytes: has_obs is written as
// dwords throughout, is_bad as dwords where the source happens to sit at the same offset within a dword, else byte by byte (no unaligned wide access);
// the ragged ends are copied as bytes by the first 8 threads of the frame.  grid (ceil(largest M / 4 / 256) >= 1, B), 256 threads
__global__ void __launch_bounds__(256) k_map_set_flags(const SetFlagRec* __restrict__ recs, uint8_t* __restrict__ bad, uint8_t* __restrict__ obs) {
    const SetFlagRec R = recs[blockIdx.y];
    const uint8_t* __restrict__ src = R.seen;
    uint8_t* db = bad + (size_t)R.off; uint8_t* dobs = obs + (size_t)R.off;
    const int M = R.M;
    const int head = imin((int)((4u - (unsigned)((uintptr_t)db & 3u)) & 3u), M), nw = (M - head) >> 2, tail0 = head + 4 * nw;
    const bool agree = (((uintptr_t)src ^ (uintptr_t)db) & 3u) == 0;
    const int w = (int)(blockIdx.x * 256u + threadIdx.x);
    if (w < nw) {
        const int o = head + 4 * w;
        *(uint32_t*)(dobs + o) = 0x01010101u;
        if (agree) *(uint32_t*)(db + o) = *(const uint32_t*)(src + o);
        else { db[o] = src[o]; db[o + 1] = src[o + 1]; db[o + 2] = src[o + 2]; db[o + 3] = src[o + 3]; }
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) {
        const int k = (int)threadIdx.x, o = k < 4 ? k : tail0 + k - 4;
        if (k < 4 ? k < head : o < M) { db[o] = src[o]; dobs[o] = 1; }
    }
}

// `assigned` of such a batch as map slots: out = the slot of the set's point a for a >= 0, negative entries as they are.  (An index outside the set cannot
// come out of the accept kernels; it would read as -1 rather than reach past the list.)  S entries per frame.  grid (ceil(S / 256), B), 256 threads
__global__ void __launch_bounds__(256) k_assigned_slots(const SetFlagRec* __restrict__ recs, const int* __restrict__ assigned, int S, int* __restrict__ out) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= S) return;
    const SetFlagRec R = recs[blockIdx.y];
    const size_t o = (size_t)blockIdx.y * (size_t)S + (size_t)i;
    const int a = assigned[o];
    out[o] = a < 0 ? a : (a < R.M ? R.slots[a] : -1);
}

// ---- the exclusions of a Fuse / Sim3 projection batch read from the map (orbm_fuse_candidates_batch_map / orbm_search_by_projection_sim3_batch_map) ----
// skip[k][i] of the host-fed calls - `pMP->isBad() || pMP->IsInKeyFrame(pKF)` (src/ORBmatcher.cc:1366-1375), spAlreadyFound (:512-525, :561, :633-645,
// :1561, :1575) - written where those calls upload it, in O(M + K M + listed slots): a table by slot names a position of the set, the targets' lists are
// looked up in it.  table[slot] holds top - (the first position of the set that is this slot), offered with atomicMax as the first-occurrence stamps of
// k_map_stamp are: this call's offers lie in (base, top], top = base + M, whatever an earlier call left is <= base and reads as "not in the set", and
// nothing is cleared between calls.  Three launches, each after the other has ended:
//   k_map_set_table    position i offers itself to its slot's entry and writes the slot's bad flag to skip[k][i] of kSkipTargets targets
//   k_map_skip_listed  entry j of target k's list (a key-frame row, a found list; -1 and slots outside the set fall through) stores 1 at skip[k][position]:
//                      every writer of a byte stores the same value
//   k_map_skip_dups    a position that is not its slot's first takes the first one's flag (orbm_map_select allows a slot at several positions); the
//                      bytes read here (first positions) are not written here
// grid (ceil(M / 256), ceil(K / kSkipTargets)), 256 threads
__global__ void __launch_bounds__(256) k_map_set_table(int M, int K, const int* __restrict__ slots, const uint8_t* __restrict__ state, unsigned* __restrict__ table,
                                                       unsigned top, uint8_t* __restrict__ skip) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= M) return;
    const int slot = slots[i];
    if (blockIdx.y == 0) atomicMax(&table[slot], top - (unsigned)i);
    const uint8_t bad = (uint8_t)(state[slot] != kMapPresent);
    const int k0 = (int)blockIdx.y * kSkipTargets, k1 = imin(K, k0 + kSkipTargets);
    for (int k = k0; k < k1; k++) skip[(size_t)k * (size_t)M + (size_t)i] = bad;
}

// grid (ceil(longest list / 256), K), 256 threads
__global__ void __launch_bounds__(256) k_map_skip_listed(const MapSkipRec* __restrict__ recs, const int* __restrict__ lists, int M, const unsigned* __restrict__ table,
                                                         unsigned base, unsigned top, uint8_t* __restrict__ skip) {
    const MapSkipRec R = recs[blockIdx.y];
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j >= R.n) return;
    const int slot = lists[(size_t)R.off + (size_t)j];
    if (slot < 0) return;
    const unsigned t = table[slot], p = top - t;
    if (t > base && p < (unsigned)M) skip[(size_t)blockIdx.y * (size_t)M + (size_t)p] = 1;
}

// grid as k_map_set_table
__global__ void __launch_bounds__(256) k_map_skip_dups(int M, int K, const int* __restrict__ slots, const unsigned* __restrict__ table, unsigned top,
                                                       uint8_t* __restrict__ skip) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= M) return;
    const unsigned first = top - table[slots[i]];
    if (first >= (unsigned)i) return;                               // (its slot's first position; a later one cannot be the first)
    const int k0 = (int)blockIdx.y * kSkipTargets, k1 = imin(K, k0 + kSkipTargets);
    for (int k = k0; k < k1; k++) {
        const size_t o = (size_t)k * (size_t)M;
        if (skip[o + first]) skip[o + (size_t)i] = 1;
    }
}

// pKF->GetMapPoint(bestIdx) of the Fuse replay (:1505-1526, :1655-1668) as a slot: entry feat0 + bestIdx of the target's row if that slot holds a point
// that is not bad, -2 if it holds a bad one (the replay does nothing), -1 if the entry is -1 or its slot holds nothing (AddObservation / AddMapPoint),
// and -1 where best_idx is.  grid (ceil(M / 256), K), 256 threads
__global__ void __launch_bounds__(256) k_fuse_kf_slots(const MapSkipRec* __restrict__ recs, const int* __restrict__ kf_slots, int M, const uint8_t* __restrict__ state,
                                                       const int* __restrict__ best_idx, int* __restrict__ kf_slot) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= M) return;
    const size_t o = (size_t)blockIdx.y * (size_t)M + (size_t)i;
    const int b = best_idx[o];
    int out = -1;
    if (b >= 0) {
        const MapSkipRec R = recs[blockIdx.y];
        const int slot = kf_slots[(size_t)R.off + (size_t)R.feat0 + (size_t)b];
        if (slot >= 0) { const uint8_t st = state[slot]; out = st == kMapPresent ? slot : (st & kMapPresent) ? -2 : -1; }
    }
    kf_slot[o] = out;
}

// ---- the matched pairs of a Fuse batch as one list (orbm_fuse_pairs_batch / orbm_fuse_pairs_batch_map) --------------------------------------------
// Behind k_fuse_candidates, on its dense best_idx[K][M]: the pairs with best_idx >= 0, target by target and inside a target by position - the order the
// replay visits them in.  As the local-map build compacts (k_map_compact / k_map_scan): a chunk is kPairChunk positions of one target, chunk c of target k is
// number k * gridDim.x + c, so the order of the numbers is the order of the list; its pairs are counted with wave ballots, the counts are scanned, and the
// same ballots rank each pair inside its chunk.  No cursor is shared, so the order does not depend on which workgroup runs first.
//   k_fuse_pairs (chunk_off == nullptr)   chunk_cnt[chunk], nothing else
//   k_fuse_pair_scan_tiles                a tile is kPairTile chunks, one wave: chunk_off = exclusive scan inside the tile, tile_sum = the tile's pairs
//   k_fuse_pair_scan_sums                 tile_off = exclusive scan of tile_sum, tile_off[ntiles] = all pairs; one workgroup, a run of tiles per thread
//   k_fuse_pairs (chunk_off != nullptr)   start[k] = the offset of target k's first chunk, start[K] = all pairs; if they fit in cap, the record of every pair

// pKF->GetMapPoint(feat) of the replay for one pair, by the rule of k_fuse_kf_slots: the slot, -2 for a bad point, -1 for no point
__device__ __forceinline__ int fuse_pair_kf_slot(const MapSkipRec& R, const int* __restrict__ kf_slots, const uint8_t* __restrict__ state, int feat) {
    const int slot = kf_slots[(size_t)R.off + (size_t)R.feat0 + (size_t)feat];
    if (slot < 0) return -1;
    const uint8_t st = state[slot];
    if (!(st & kMapPresent)) return -1;
    return (st & kMapBad) ? -2 : slot;
}

// grid (ceil(M / kPairChunk), K), kPairChunk threads.  A record is O.fields ints: position, feature, then what the caller asked for (FusePairOut)
__global__ void __launch_bounds__(kPairChunk) k_fuse_pairs(int M, const int* __restrict__ best_idx, const int* __restrict__ best_dist, int* __restrict__ chunk_cnt,
                                                           const int* __restrict__ chunk_off, const int* __restrict__ tile_off, int ntiles, int cap,
                                                           int* __restrict__ start, const MapSkipRec* __restrict__ recs, const int* __restrict__ kf_slots,
                                                           const uint8_t* __restrict__ state, const int* __restrict__ set_slots, FusePairOut O) {
    __shared__ int wave_cnt[kPairChunk / 64];
    const int k = (int)blockIdx.y, i = (int)(blockIdx.x * (unsigned)kPairChunk + threadIdx.x);
    const size_t o = (size_t)k * (size_t)M + (size_t)i;
    const int feat = i < M ? best_idx[o] : -1;
    const bool keep = feat >= 0;
    const unsigned long long bal = __ballot(keep);
    const int lane = lane_id(), wave = wave_id();
    if (lane == 0) wave_cnt[wave] = __popcll(bal);
    __syncthreads();
    const int chunk = k * (int)gridDim.x + (int)blockIdx.x;
    if (!chunk_off) {
        if (threadIdx.x == 0) { int c = 0; for (int w = 0; w < kPairChunk / 64; w++) c += wave_cnt[w]; chunk_cnt[chunk] = c; }
        return;
    }
    const int at0 = tile_off[chunk / kPairTile] + chunk_off[chunk], total = tile_off[ntiles];
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) start[k] = at0;
        if (chunk == 0) start[gridDim.y] = total;
    }
    if (!keep || total > cap) return;                               // (nothing is truncated: a list that does not fit is not written at all)
    int at = at0 + __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) at += wave_cnt[w];
    if (at >= total) return;                                        // (cannot happen: the offsets are the scan of these counts; it keeps the store inside the list)
    int* __restrict__ r = O.rec + (size_t)at * (size_t)O.fields;
    r[0] = i; r[1] = feat;
    if (O.dist >= 0) r[O.dist] = best_dist[o];
    if (O.point_slot >= 0) r[O.point_slot] = set_slots[i];
    if (O.kf_slot >= 0) r[O.kf_slot] = fuse_pair_kf_slot(recs[k], kf_slots, state, feat);
}

// grid (ceil(n / 256)), 256 threads: four tiles
__global__ void __launch_bounds__(256) k_fuse_pair_scan_tiles(int n, const int* __restrict__ chunk_cnt, int* __restrict__ chunk_off, int* __restrict__ tile_sum) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x), lane = lane_id();
    const int v = i < n ? chunk_cnt[i] : 0;
    const int incl = wave_incl_scan(v);
    if (i < n) chunk_off[i] = incl - v;
    if (lane == 63 && i - 63 < n) tile_sum[i / kPairTile] = incl;
}

// one workgroup of 256 threads: thread t sums tiles [t R, (t + 1) R), R = ceil(ntiles / 256) (at most 2^20 + 65535 chunks in a call: R <= 69), the sums are
// scanned over the workgroup, and each thread writes its run
__global__ void __launch_bounds__(256) k_fuse_pair_scan_sums(int ntiles, const int* __restrict__ tile_sum, int* __restrict__ tile_off) {
    __shared__ int scratch[17];
    const int R = (ntiles + 255) / 256, j0 = (int)threadIdx.x * R, j1 = imin(ntiles, j0 + R);
    int s = 0;
    for (int j = j0; j < j1; j++) s += tile_sum[j];
    int total;
    int run = block_excl_scan(s, &total, scratch);
    for (int j = j0; j < j1; j++) { run += tile_sum[j]; tile_off[j] = run - tile_sum[j]; }
    if (threadIdx.x == 0) tile_off[ntiles] = total;
}

// orbm_map_edit_keyframes: entry feat[j] of row row[j] becomes slot[j] (the host refuses two edits of one entry, so no two stores meet).
// grid (ceil(n / 256)), 256 threads
__global__ void __launch_bounds__(256) k_map_edit_rows(int n, const int* __restrict__ row, const int* __restrict__ feat, const int* __restrict__ slot,
                                                       int* __restrict__ kf_slots, int row_cap) {
    const int j = (int)(blockIdx.x * 256u + threadIdx.x);
    if (j < n) kf_slots[(size_t)row[j] * (size_t)row_cap + (size_t)feat[j]] = slot[j];
}

// ---- the stereo map points a key frame is born with (orbm_map_stereo_points) ----------------------------------------------------------------------
// Tracking::CreateNewKeyFrame (src/Tracking.cc:3868-3960) and Tracking::UpdateLastFrame (:3264-3341) sort the features with a positive depth by
// (depth, index), walk the sorted list and stop behind the first entry that is farther than mThDepth once more than `max_points` entries were visited; an
// entry whose feature keeps its map point is visited and counted, every other one gets a new point.
constexpr int kStereoSelectThreads = 256;
// Where the flagged threads of a workgroup stand among themselves, in thread order: wave ballots rank a lane inside its wave, the waves' counts are summed
// in LDS (wave_cnt: one int per wave).  Every thread calls; two barriers.  No counter is shared, so the order is the threads'.
__device__ __forceinline__ int block_ballot_rank(bool flag, int* total, int* wave_cnt) {
    const unsigned long long bal = __ballot(flag);
    const int lane = lane_id(), wave = wave_id();
    if (lane == 0) wave_cnt[wave] = __popcll(bal);
    __syncthreads();
    int at = __popcll(bal & ((1ull << lane) - 1ull)), tot = 0;
    for (int w = 0; w < kStereoSelectThreads / 64; w++) { const int c = wave_cnt[w]; if (w < wave) at += c; tot += c; }
    __syncthreads();
    *total = tot;
    return at;
}

// Phase 1, one workgroup per frame: the candidates (mvDepth[i] > 0) become keys `depth bits << 32 | i` in LDS - positive floats order as their bit
// patterns, so the keys order as std::sort orders pair<float, int>, a total order -, a bitonic network sorts them (padded to a power of two with keys
// above every real one), the stop rule cuts the prefix, and the entries that create a point are ranked in list order.  counts[2 b] = points created,
// counts[2 b + 1] = entries processed; feat_all[b * cap + j] = feature of the j-th created point.  More candidates than the sort has room for
// (P.sort_cap keys of dynamic LDS): counts = {-1, candidates}, nothing else is written.  grid (B), kStereoSelectThreads threads, 8 * P.sort_cap bytes
__global__ void __launch_bounds__(kStereoSelectThreads) k_map_stereo_select(const StereoPointsRec* __restrict__ recs, StereoPointsParams P,
                                                                            const uint8_t* __restrict__ keeps_all, int* __restrict__ feat_all,
                                                                            int* __restrict__ counts) {
    ORBX_DYN_SMEM(smem);
    unsigned long long* keys = (unsigned long long*)smem;
    __shared__ int wave_cnt[kStereoSelectThreads / 64];
    __shared__ unsigned wave_stop[kStereoSelectThreads / 64];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const StereoPointsRec& R = recs[b];
    const int N = imax(0, imin(*R.n, P.cap));
    int nc = 0;
    for (int base = 0; base < N; base += kStereoSelectThreads) {
        const int i = base + tid;
        const float d = i < N ? R.depth[i] : 0.0f;
        const bool cand = d > 0.0f;                                  // `if(z>0)`, :3880 / :3274
        int tot;
        const int at = nc + block_ballot_rank(cand, &tot, wave_cnt);
        if (cand && at < P.sort_cap) keys[at] = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(unsigned)i;
        nc += tot;
    }
    if (nc > P.sort_cap) {
        if (tid == 0) { counts[2 * b] = -1; counts[2 * b + 1] = nc; }
        return;
    }
    int P2 = 1;
    while (P2 < nc) P2 <<= 1;
    for (int i = nc + tid; i < P2; i += kStereoSelectThreads) keys[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P2 >> 1); t += kStereoSelectThreads) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned long long a = keys[lo], c = keys[hi];
                if ((a > c) == ((lo & k) == 0)) { keys[lo] = c; keys[hi] = a; }
            }
            __syncthreads();
        }
    // the loop ends behind the first entry j with depth_j > mThDepth && nPoints > max_points, nPoints = j + 1 (:3951-3955 / :3333-3337)
    unsigned stop = (unsigned)nc;
    for (int j = tid; j < nc; j += kStereoSelectThreads)
        if (__uint_as_float((unsigned)(keys[j] >> 32)) > P.th_depth && j + 1 > P.max_points) { stop = (unsigned)(j + 1); break; }
    stop = wave_min_u32(stop);
    if (lane_id() == 0) wave_stop[wave_id()] = stop;
    __syncthreads();
    for (int w = 0; w < kStereoSelectThreads / 64; w++) stop = wave_stop[w] < stop ? wave_stop[w] : stop;
    const int processed = (int)stop;
    const uint8_t* __restrict__ keeps = R.keeps_off >= 0 ? keeps_all + R.keeps_off : nullptr;
    int* __restrict__ feat = feat_all + (size_t)b * (size_t)P.cap;
    int created = 0;
    for (int base = 0; base < processed; base += kStereoSelectThreads) {
        const int j = base + tid;
        const int f = j < processed ? (int)(unsigned)(keys[j] & 0xFFFFFFFFull) : 0;
        const bool create = j < processed && !(keeps && keeps[f]);
        int tot;
        const int at = created + block_ballot_rank(create, &tot, wave_cnt);
        if (create) feat[at] = f;                                    // (at < processed <= N <= P.cap)
        created += tot;
    }
    if (tid == 0) { counts[2 * b] = created; counts[2 * b + 1] = processed; }
}

// Phase 2: the j-th created point of frame b goes to slot free_all[free_off + j].  Frame::UnprojectStereo (src/Frame.cc:1396-1409), then the fields as
// MapPoint(Pos, pMap, pFrame, idxF) computes them (P.mode 1, src/MapPoint.cc:90-128, Nleft == -1) or as MapPoint(Pos, pKF, pMap) + AddObservation +
// UpdateNormalAndDepth leave them for a point with one observation (P.mode 0, :567-642: normal = (0 + normali / |normali|) / 1, which turns a -0 into
// +0) - in the reference's fp32 statements, unfused; the matrix product as Eigen sums it (sophus_action.h).  Four lanes per point as k_map_scatter: all
// four compute the point, lane q stores two of the eight floats, lanes 0 and 1 move the descriptor row in two 16-byte accesses, lane 0 marks the slot
// present and not bad, lane 2 enters the slot in the row, lane 3 lists the feature in the call's compacted output (its frame's part starts at the sum of
// the earlier frames' counts).  The host has refused duplicate slots and rows, so no two stores meet.  grid (ceil(4 x most points / 256), B), 256 threads
__global__ void __launch_bounds__(256) k_map_stereo_write(const StereoPointsRec* __restrict__ recs, StereoPointsParams P, const int* __restrict__ free_all,
                                                          const int* __restrict__ feat_all, const int* __restrict__ counts, MapStore S,
                                                          int* __restrict__ kf_slots, int row_cap, int* __restrict__ out_feat) {
    const int b = (int)blockIdx.y;
    const StereoPointsRec& R = recs[b];
    const int t = (int)(blockIdx.x * 256u + threadIdx.x), j = t >> 2, q = t & 3;
    int before = 0;
    for (int k = lane_id(); k < b; k += 64) before += counts[2 * k];
    before = wave_sum(before);
    if (j >= counts[2 * b]) return;
    const int i = feat_all[(size_t)b * (size_t)P.cap + (size_t)j];
    const size_t slot = (size_t)free_all[R.free_off + j];
    const KeyPointRec* __restrict__ kp = R.kps + i;
    const float z = R.depth[i], u = kp->x, v = kp->y;
    const float x = __fmul_rn(__fmul_rn(__fsub_rn(u, P.cx), z), P.invfx), y = __fmul_rn(__fmul_rn(__fsub_rn(v, P.cy), z), P.invfy);
    float pos[3];
    eig_rt3(R.Rwc, R.Ow, x, y, z, pos);                              // x3D = mRwc * x3Dc + mOw
    const float o0 = __fsub_rn(pos[0], R.Ow[0]), o1 = __fsub_rn(pos[1], R.Ow[1]), o2 = __fsub_rn(pos[2], R.Ow[2]);
    const float dist = sqrtf(eig_dot3(o0, o1, o2, o0, o1, o2));
    float n0 = __fdiv_rn(o0, dist), n1 = __fdiv_rn(o1, dist), n2 = __fdiv_rn(o2, dist);
    if (P.mode == 0) {
        n0 = __fdiv_rn(__fadd_rn(0.0f, n0), 1.0f); n1 = __fdiv_rn(__fadd_rn(0.0f, n1), 1.0f); n2 = __fdiv_rn(__fadd_rn(0.0f, n2), 1.0f);
    }
    const float max_d = __fmul_rn(dist, pick(P.scale, kp->octave)), min_d = __fdiv_rn(max_d, P.scale_top);
    if (q < 2) ((int4*)S.desc)[2 * slot + (size_t)q] = ((const int4*)R.desc)[2 * (size_t)i + (size_t)q];
    if (q == 0) { S.pos[3 * slot] = pos[0]; S.pos[3 * slot + 1] = pos[1]; S.state[slot] = (uint8_t)kMapPresent; }
    else if (q == 1) { S.pos[3 * slot + 2] = pos[2]; S.normal[3 * slot] = n0; }
    else if (q == 2) { S.normal[3 * slot + 1] = n1; S.normal[3 * slot + 2] = n2; if (R.row >= 0) kf_slots[(size_t)R.row * (size_t)row_cap + (size_t)i] = (int)slot; }
    else { S.min_d[slot] = min_d; S.max_d[slot] = max_d; out_feat[before + j] = i; }
}

// ---- key frames made from extracted frames (orbm_keyframe_create_extracted / _rig_extracted) ----------------------------------------------------
// What the host must know of every frame before it can allocate: out[3 j ..] = features, FeatureVector nodes, FeatureVector entries of record j
// (the counts are clamped to what the arrays can hold; the host refuses a FeatureVector that does not fit its frame).  grid (ceil(n / 64)), 64 threads
__global__ void __launch_bounds__(64) k_keyframe_counts(const KfSnapRec* __restrict__ recs, int n, int* __restrict__ out) {
    const int j = (int)(blockIdx.x * 64u + threadIdx.x);
    if (j >= n) return;
    const KfSnapRec R = recs[j];
    const int N = imin(*R.n_l, R.cap) + (R.kps_r ? imin(*R.n_r, R.cap) : 0);
    const int rows = R.kps_r ? 2 * R.cap : R.cap;                  // per-frame stride of the transform's arrays
    int nn = 0, nf = 0;
    if (R.node_id) { nn = imin(*R.fv_nodes, rows); if (nn < 0) nn = 0; nf = R.fv_start[nn]; }
    out[3 * j] = N; out[3 * j + 1] = nn; out[3 * j + 2] = nf;
}

// The copy: every section of the key frames' blocks in one launch.  grid (chunks, n), 256 threads; the workgroups of a key frame stride over each section.
// Keypoint records are 28 B and a frame's rows start at a multiple of 28 B: they move as flat dwords (camera 2's of a rig frame behind camera 1's);
// descriptor rows are 32 B at 32 B multiples on both sides: two 16 B accesses per row; uRight, node ids, offsets and feature indices start at
// dword multiples in the source: dwords.  node_of_feat is the inverse of the CSR with -1 for the features in no node: filling and scattering must not
// overlap, so the first workgroup of a key frame does both around a barrier (a few thousand entries) and the other workgroups never touch that section.
// The entry behind the node ids and behind the feature indices (the sections hold one more than they need) is written as 0.
__global__ void __launch_bounds__(256) k_keyframe_snapshot(const KfSnapRec* __restrict__ recs) {
    const KfSnapRec R = recs[blockIdx.y];
    const int t0 = (int)(blockIdx.x * 256u + threadIdx.x), step = (int)(gridDim.x * 256u);
    const int N = R.N, N1 = N > 0 ? N : 1, nn = R.nn, nf = R.nf;
    const int nl = R.kps_r ? imin(imin(*R.n_l, R.cap), N) : N;
    {
        uint32_t* d = (uint32_t*)R.dst;
        const uint32_t *s1 = (const uint32_t*)R.kps, *s2 = (const uint32_t*)R.kps_r;
        for (int i = t0; i < 7 * N; i += step) d[i] = i < 7 * nl ? s1[i] : s2[i - 7 * nl];
        for (int i = t0; i < N; i += step) R.angle[i] = i < nl ? R.kps[i].angle : R.kps_r[i - nl].angle;
    }
    {
        const int4* s = (const int4*)R.desc; int4* d = (int4*)(R.dst + R.o_desc);
        for (int i = t0; i < 2 * N; i += step) d[i] = s[i];
    }
    {
        float* d = (float*)(R.dst + R.o_ur);
        for (int i = t0; i < N1; i += step) d[i] = (R.ur && i < N) ? R.ur[i] : -1.0f;
    }
    {
        uint32_t* dn = (uint32_t*)(R.dst + R.o_nid); int* ds = (int*)(R.dst + R.o_st); int* df = (int*)(R.dst + R.o_ft);
        for (int i = t0; i <= nn; i += step) { dn[i] = i < nn ? R.node_id[i] : 0u; ds[i] = nn > 0 ? R.fv_start[i] : 0; }
        for (int i = t0; i <= nf; i += step) df[i] = i < nf ? R.fv_feat[i] : 0;
    }
    if (blockIdx.x != 0) return;
    int* nof = (int*)(R.dst + R.o_nof);
    for (int i = (int)threadIdx.x; i < N1; i += 256) nof[i] = -1;
    __syncthreads();
    for (int k = (int)threadIdx.x; k < nf; k += 256) {
        int lo = 0, hi = nn;                                        // the node a with fv_start[a] <= k < fv_start[a + 1]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (R.fv_start[mid] <= k) lo = mid; else hi = mid; }
        const int f = R.fv_feat[k];
        if ((unsigned)f < (unsigned)N) nof[f] = lo;
    }
}

}  // namespace orbx
