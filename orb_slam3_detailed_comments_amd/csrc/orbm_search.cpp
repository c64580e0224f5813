// orbm_search.cpp — host side of the guided searches (include/orbx.h "Guided searches").  All Hamming distances and all window / level / gate /
// epipolar tests run on the GPU; the host uploads the SoA views, launches the kernels of k_search.hip and - where the reference's acceptance loop is
// order-dependent (an assignment for one map point changes the candidate set of the next) - replays it over the device-computed candidate lists,
// comparing precomputed integers in the reference's sequence.  Map of the file:
//   shared pieces           Bump / Packer (block layout, one staged upload), upload_frame, the window search with its candidate pool (pooled_area_search), the replay
//                           helpers (Cands, scan_best, scan_best2, RotHist, for_each_common_node, fill_kb8)
//   single-frame searches   GetFeaturesInArea, SearchByProjection(Frame, MapPoints), isInFrustum (one camera and rig), SearchLocalPoints,
//                           SearchByProjection(Frame, Frame), SearchForTriangulation, SearchByBoW, SearchForInitialization, the projected-point searches
//                           (Sim3, key frame, Fuse, SearchBySim3), DistinctiveDescriptors, the two-camera (fisheye) forms
//   resident objects        orbm_points (map points), orbm_keyframe (key frames, with the grids the Fuse batch builds for them) and the searches that read them;
//                           orbm_fuse_candidates_batch and orbm_search_by_projection_sim3_batch (one point set against many key frames) stand with the single
//                           Fuse search
//   batched routes          frames of the last extraction: SearchLocalPoints, SearchByProjection(last frame / key frame), SearchByBoW; one fetch
//   rig routes              the same for two-camera frames (two handles), fetched through the same core
//   resident map            orbm_map: the map-point store by slot, key-frame rows of slots, Tracking::UpdateLocalPoints for a batch of frames built on the
//                           device into orbm_points sets that every search above takes; the tracking searches, and the Fuse / Sim3 batches, fed from it
// The line numbers in the comments point into the reference's src/ORBmatcher.cc unless another file is named.
#include <mutex>
#include "orbx_internal.h"

using namespace orbx;

namespace {

const int TH_HIGH = 100, TH_LOW = 50, HISTO_LENGTH = 30;   // src/ORBmatcher.cc:35-37
const int kGridColsHost = 64, kGridRowsHost = 48;          // FRAME_GRID_COLS / FRAME_GRID_ROWS, include/Frame.h:44-45

struct DeviceFrame {
    const KeyPointRec* kps; const unsigned long long* desc; const float* ur; const int* cell_start; const int* cell_items;
    GridParams g;
};

// scratch slots in orbx_extractor::d_sr / d_si
enum { SR_KPS = 0, SR_DESC, SR_UR, SR_QUERY, SR_QDESC, SR_ENTRIES, SR_KPS2, SR_DESC2, SR_UR2, SR_HASMP2, SR_ITEMS, SR_SPARE };
enum { SI_CELLOF = 0, SI_CELLSTART, SI_CELLITEMS, SI_QSTART, SI_QCOUNT, SI_COUNTER, SI_FEAT2, SI_BEST };

int upload(orbx_extractor* h, int slot, const void* src, size_t bytes) {
    if (h->d_sr[slot].ensure(bytes + 16)) return -1;
    return rt::copy_h2d(h->d_sr[slot].p, src, bytes, h->s0);
}

// Per call the window searches move: frame (keypoints | descriptors | uRight) and queries (AreaQuery | descriptors) up, the candidate
// lists down.  Each direction is ONE async copy between a pinned staging buffer and one device buffer (a call is latency-bound: with a
// dozen small pageable copies the driver calls cost more than the kernels).
inline size_t al16(size_t v) { return (v + 15) & ~(size_t)15; }

// lays 16-byte aligned parts out one behind the other: take() returns the offset of the next one
struct Bump {
    size_t o;
    explicit Bump(size_t start = 0) : o(start) {}
    size_t take(size_t bytes) { const size_t at = o; o += al16(bytes); return at; }
};

// several host arrays -> one pinned staging buffer -> one async copy into a scratch slot (h_packA -> d_sr[SR_KPS] unless the caller chooses others).
// add() copies an array, fill() writes `bytes` of one value, room() reserves device space behind the upload (after the last add / fill);
// each returns the part whose device address dev() / out() gives after flush()
struct Packer {
    struct Part { const void* src; size_t bytes; int value; size_t off; };
    orbx_extractor* h; HostBuf<uint8_t>& stage; int slot; std::vector<Part> parts; Bump lay; size_t uploaded = 0;
    explicit Packer(orbx_extractor* hh) : h(hh), stage(hh->h_packA), slot(SR_KPS) {}
    Packer(orbx_extractor* hh, HostBuf<uint8_t>& st, int sl) : h(hh), stage(st), slot(sl) {}
    size_t part(const void* src, size_t bytes, int value) { parts.push_back({src, bytes, value, lay.take(bytes ? bytes : 1)}); uploaded = lay.o; return parts.size() - 1; }
    size_t add(const void* src, size_t bytes) { return part(src, bytes, 0); }
    size_t fill(int value, size_t bytes) { return part(nullptr, bytes, value); }
    size_t room(size_t bytes) { parts.push_back({nullptr, 0, 0, lay.take(bytes)}); return parts.size() - 1; }
    int flush() {                                                   // -1: an allocation failed, -2: the copy
        if (stage.ensure(uploaded + 16) || h->d_sr[slot].ensure(lay.o + 16)) return -1;
        for (const Part& p : parts) { if (p.src) memcpy(stage.p + p.off, p.src, p.bytes); else if (p.bytes) memset(stage.p + p.off, p.value, p.bytes); }
        return rt::copy_h2d(h->d_sr[slot].p, stage.p, uploaded, h->s0) ? -2 : 0;
    }
    template <typename T> const T* dev(size_t part) const { return (const T*)(h->d_sr[slot].p + parts[part].off); }
    template <typename T> T* out(size_t part) const { return (T*)(h->d_sr[slot].p + parts[part].off); }
};
const char* upload_error(int e) { return e == -1 ? "upload/allocation failed" : "upload failed"; }

int frame_check(const OrbmFrameView* F) {
    if (!F || F->N < 0 || (F->N > 0 && (!F->keys_un || !F->desc))) return fail(ORBX_E_ARG, "bad frame view");
    if (F->N >= 65535) return fail(ORBX_E_ARG, "too many keypoints");
    return ORBX_OK;
}
// the frame (keypoints | descriptors | uRight, -1 where the frame has none) and what more() adds to pk behind it go up in one copy; then the frame's grid is built
template <typename More>
int upload_frame(orbx_extractor* h, const OrbmFrameView* F, DeviceFrame* D, Packer& pk, const More& more) {
    int rc = frame_check(F); if (rc) return rc;
    const int N = F->N;
    std::vector<float> mono;
    if (!F->u_right) mono.assign(N > 0 ? N : 1, -1.0f);
    const size_t pkp = pk.add(F->keys_un, sizeof(KeyPointRec) * (size_t)N), pdesc = pk.add(F->desc, 32 * (size_t)N),
                 pur = F->u_right ? pk.add(F->u_right, sizeof(float) * (size_t)N) : pk.add(mono.data(), sizeof(float) * mono.size());
    more();
    if (h->d_si[SI_CELLOF].ensure(N + 1) | h->d_si[SI_CELLSTART].ensure(64 * 48 + 2) | h->d_si[SI_CELLITEMS].ensure(N + 1) | h->d_si[SI_COUNTER].ensure(4))
        return fail(ORBX_E_DEVICE, "upload/allocation failed");
    if (int e = pk.flush()) return fail(ORBX_E_DEVICE, "%s", upload_error(e));
    D->kps = pk.dev<KeyPointRec>(pkp); D->desc = pk.dev<unsigned long long>(pdesc); D->ur = pk.dev<float>(pur);
    memset(&D->g, 0, sizeof D->g);
    D->g.min_x = F->min_x; D->g.min_y = F->min_y; D->g.gw_inv = F->grid_w_inv; D->g.gh_inv = F->grid_h_inv;
    const dim3 one(1, 1, 1), blkg(kGridThreads, 1, 1);
    ORBX_LAUNCH(k_grid_build, one, blkg, 0, h->s0, D->kps, N, D->g, h->d_si[SI_CELLOF].p, h->d_si[SI_CELLSTART].p, h->d_si[SI_CELLITEMS].p, (const int*)nullptr, 0);
    D->cell_start = h->d_si[SI_CELLSTART].p; D->cell_items = h->d_si[SI_CELLITEMS].p;
    return ORBX_OK;
}
int upload_frame(orbx_extractor* h, const OrbmFrameView* F, DeviceFrame* D) { Packer pk(h); return upload_frame(h, F, D, pk, [] {}); }

void fill_frustum_params(const OrbmFrustumView* V, float cos_limit, float th, int far_points, float th_far, FrustumParams* Fp) {
    memset(Fp, 0, sizeof *Fp);
    memcpy(Fp->Rcw, V->Rcw, sizeof Fp->Rcw); memcpy(Fp->tcw, V->tcw, sizeof Fp->tcw); memcpy(Fp->Ow, V->Ow, sizeof Fp->Ow); memcpy(Fp->qcw, V->qcw, sizeof Fp->qcw);
    memcpy(Fp->cam, V->cam, sizeof Fp->cam); Fp->kb8 = V->camera_type == 1;
    Fp->min_x = V->min_x; Fp->max_x = V->max_x; Fp->min_y = V->min_y; Fp->max_y = V->max_y; Fp->mbf = V->mbf; Fp->log_scale_factor = V->log_scale_factor; Fp->nlevels = V->nlevels;
    for (int l = 0; l < V->nlevels; l++) Fp->scale_factors[l] = V->scale_factors[l];
    Fp->cos_limit = cos_limit; Fp->th = th; Fp->th_far = th_far; Fp->far_points = far_points;
}

// ---- the candidate lists of a window search, and the pieces of the replays over them ----
// query q owns `count[q]` entries from `start[q]` on, two ints each: {keypoint, dist | octave << 16}, in the order of the reference's GetFeaturesInArea
struct Csr;
struct Cands {
    const int *start = nullptr, *count = nullptr, *ent = nullptr; int total = 0;
    Cands() {}
    Cands(const int* s, const int* c, const int* e, int t) : start(s), count(c), ent(e), total(t) {}     // the pinned block a search came back in
    Cands(const Csr& c);
    int idx(int q, int k) const { return ent[2 * ((size_t)start[q] + k)]; }
    int dist(int q, int k) const { return ent[2 * ((size_t)start[q] + k) + 1] & 0xFFFF; }
    int level(int q, int k) const { return ent[2 * ((size_t)start[q] + k) + 1] >> 16; }
};
// a copy of the lists, for the replays that hold two searches at a time (the pinned block is overwritten by the handle's next search)
struct Csr {
    std::vector<int> start, count, ent;
    void copy(const Cands& c, int Q) { start.assign(c.start, c.start + Q); count.assign(c.count, c.count + Q); ent.assign(c.ent, c.ent + 2 * (size_t)c.total); ent.resize(ent.size() + 2); }
};
Cands::Cands(const Csr& c) : start(c.start.data()), count(c.count.data()), ent(c.ent.data()), total((int)c.ent.size() / 2 - 1) {}

// the nearest candidate of query q on a free keypoint (occ == nullptr: on any).  off: the candidates are camera 2's, whose slots follow camera 1's Nleft
struct Best { int dist, idx; };
Best scan_best(const Cands& c, int q, const uint8_t* occ, int off = 0, int init = 256) {
    Best b = {init, -1};
    for (int k = 0; k < c.count[q]; k++) {
        const int idx = c.idx(q, k), dist = c.dist(q, k);
        if (occ && occ[idx + off]) continue;
        if (dist < b.dist) { b.dist = dist; b.idx = idx; }
    }
    return b;
}
// the two nearest with their pyramid levels, as the scan of SearchByProjection(Frame, MapPoints) keeps them (:101-140)
struct Best2 { int bestDist, bestLevel, bestDist2, bestLevel2, bestIdx; };
Best2 scan_best2(const Cands& c, int q, const uint8_t* occ, int off = 0) {
    int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
    for (int k = 0; k < c.count[q]; k++) {
        const int idx = c.idx(q, k);
        if (occ && occ[idx + off]) continue;
        const int dist = c.dist(q, k), level = c.level(q, k);
        if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = level; bestIdx = idx; }
        else if (dist < bestDist2) { bestLevel2 = level; bestDist2 = dist; }
    }
    return {bestDist, bestLevel, bestDist2, bestLevel2, bestIdx};
}

// the rotation-consistency check: matches vote with their angle difference, those outside the three strongest bins are reset (:2118-2123, :2161-2176)
class RotHist {
    std::vector<int> rotHist[HISTO_LENGTH];
    // ORBmatcher::ComputeThreeMaxima, src/ORBmatcher.cc:2335-2377
    static void three_maxima(const std::vector<int>* histo, int L, int& ind1, int& ind2, int& ind3) {
        int max1 = 0, max2 = 0, max3 = 0;
        for (int i = 0; i < L; i++) {
            const int s = (int)histo[i].size();
            if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
            else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
            else if (s > max3) { max3 = s; ind3 = i; }
        }
        if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
        else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
    }
    static int rot_bin(float a1, float a2) {    // :2118-2123; the 1/HISTO_LENGTH factor is the reference's (kept on purpose)
        const float factor = 1.0f / HISTO_LENGTH;
        float rot = a1 - a2;
        if (rot < 0.0) rot += 360.0f;
        int bin = (int)round(rot * factor);
        if (bin == HISTO_LENGTH) bin = 0;
        return bin;
    }
public:
    void add(float angle1, float angle2, int id) { rotHist[rot_bin(angle1, angle2)].push_back(id); }
    // reset(id) for every id outside the three strongest bins, in bin order
    template <typename Reset> void prune(const Reset& reset) const {
        int ind1 = -1, ind2 = -1, ind3 = -1;
        three_maxima(rotHist, HISTO_LENGTH, ind1, ind2, ind3);
        for (int i = 0; i < HISTO_LENGTH; i++) {
            if (i == ind1 || i == ind2 || i == ind3) continue;
            for (int id : rotHist[i]) reset(id);
        }
    }
};

// merge-join of two FeatureVectors by node id (:1105-1286, :300-474, :917-1021): fn(a, b) for every vocabulary node that both key frames hold
template <typename Fn> void for_each_common_node(const OrbmKeyFrameView* K1, const OrbmKeyFrameView* K2, const Fn& fn) {
    int a = 0, b = 0;
    while (a < K1->fv_nodes && b < K2->fv_nodes) {
        const uint32_t na = K1->fv_node_id[a], nb = K2->fv_node_id[b];
        if (na == nb) { fn(a, b); a++; b++; }
        else if (na < nb) { while (a < K1->fv_nodes && K1->fv_node_id[a] < nb) a++; }
        else { while (b < K2->fv_nodes && K2->fv_node_id[b] < na) b++; }
    }
}
// the Kannala-Brandt half of BowParams: the camera pair of one neighbour and KF1's level variances
void fill_kb8(BowParams& P, const OrbmKB8Pair& C, const float* sigma2_1, int nlevels) {
    P.kb8 = 1; P.nleft1 = C.nleft1; P.nleft2 = C.nleft2;
    memcpy(P.cam1, C.cam1, sizeof P.cam1); memcpy(P.cam2, C.cam2, sizeof P.cam2); memcpy(P.R, C.R, sizeof P.R); memcpy(P.t, C.t, sizeof P.t);
    for (int l = 0; l < nlevels && l < kMaxLevels; l++) P.sigma2_1[l] = sigma2_1[l];
}

// the ordered loop of SearchByProjection(Frame, MapPoints) over one camera's candidates, :62-166 (a map point that is not in view, far, bad or
// on a level the frame does not have got no window: count 0); returns nmatches
int replay_mappoints(const Cands& c, int M, float nnratio, const uint8_t* has_obs, uint8_t* occ, int* assigned) {
    int nmatches = 0;
    for (int i = 0; i < M; i++) {
        if (c.count[i] == 0) continue;
        const Best2 b = scan_best2(c, i, occ);
        if (b.bestDist <= TH_HIGH) {
            if (b.bestLevel == b.bestLevel2 && b.bestDist > nnratio * b.bestDist2) continue;
            if (b.bestLevel != b.bestLevel2 || b.bestDist <= nnratio * b.bestDist2) {
                assigned[b.bestIdx] = i;
                occ[b.bestIdx] = has_obs ? has_obs[i] : 1;
                nmatches++;
            }
        }
    }
    return nmatches;
}

// ---- the window search of one frame ----
// the result block in d_sr[SR_ENTRIES] and its pinned copy in h_out: [counter 16 | start Q | count Q] | `mid` bytes of the caller's | entry pool
struct AreaBlock {
    int* counter; int* start; int* count; uint8_t* mid; int2* ent;
    AreaBlock(uint8_t* p, size_t Q, size_t mid_bytes) : counter((int*)p), start((int*)(p + 16)), count(start + Q), mid(p + al16(16 + 8 * Q)), ent((int2*)(mid + mid_bytes)) {}
};
void launch_area_search(orbx_extractor* h, const DeviceFrame& D, int Q, const AreaQuery* dq, const unsigned long long* dqd, const AreaBlock& o, size_t pool) {
    dim3 grid((Q + kAreaWaves - 1) / kAreaWaves, 1, 1), blk(64 * kAreaWaves, 1, 1);
    ORBX_LAUNCH(k_area_search, grid, blk, 0, h->s0, dq, dqd, Q, D.kps, D.ur, D.desc, D.g, D.cell_start, D.cell_items, 1, o.counter, (int)pool, o.start, o.count, o.ent);
}
// The candidate-pool protocol of the single-frame searches.  launch(block, pool) enqueues the kernels that zero the counter and fill the block
// for Q queries.  Results come back in one copy: the number of entries fetched with the header (and the caller's `mid` bytes, *mid_host
// afterwards) is a guess from the previous call, a second copy follows only if it was too small, and the pool is grown and the launch
// repeated if the pool itself overflowed (the first call of a much denser scene).  *out reads the pinned block: valid until the handle's next search.
template <typename Launch>
int pooled_area_search(orbx_extractor* h, int Q, size_t mid_bytes, const char* what, const Launch& launch, Cands* out, const uint8_t** mid_host = nullptr) {
    const size_t oent = al16(16 + 8 * (size_t)Q) + mid_bytes;       // bytes in front of the entries
    size_t pool = std::max<size_t>(h->area_pool, (size_t)Q * 48 + 1024);
    for (int attempt = 0; attempt < 2; attempt++) {
        if (h->d_sr[SR_ENTRIES].ensure(oent + pool * 8 + 16)) return fail(ORBX_E_DEVICE, "entry pool allocation failed");
        if (h->h_out.ensure(oent + pool * 8 + 16)) return fail(ORBX_E_DEVICE, "pinned allocation failed");
        h->area_pool = pool;
        uint8_t* dout = h->d_sr[SR_ENTRIES].p;
        launch(AreaBlock(dout, Q, mid_bytes), pool);
        const size_t guess = std::min(pool, std::max<size_t>(h->area_last_total + h->area_last_total / 4 + 256, 1024));
        rt::copy_d2h(h->h_out.p, dout, oent + guess * 8, h->s0);
        if (rt::stream_sync(h->s0) || rt::check_launch()) return fail(ORBX_E_DEVICE, "%s failed: %s", what, rt::last_error());
        const int total = *(const int*)h->h_out.p;
        if ((size_t)total <= pool) {
            if ((size_t)total > guess) {
                rt::copy_d2h(h->h_out.p + oent + guess * 8, dout + oent + guess * 8, ((size_t)total - guess) * 8, h->s0);
                if (rt::stream_sync(h->s0)) return fail(ORBX_E_DEVICE, "%s download failed: %s", what, rt::last_error());
            }
            h->area_last_total = (size_t)total;
            const AreaBlock host(h->h_out.p, Q, mid_bytes);
            *out = Cands(host.start, host.count, (const int*)host.ent, total);
            if (mid_host) *mid_host = host.mid;
            return ORBX_OK;
        }
        pool = (size_t)total + 1024;
    }
    return fail(ORBX_E_INTERNAL, "entry pool overflow after retry");
}
// k_area_search for host queries: they and their descriptors go up in one copy (h_packB -> d_sr[SR_QUERY])
int run_area_search(orbx_extractor* h, const DeviceFrame& D, const std::vector<AreaQuery>& qs, const uint8_t* qdesc, Cands* out) {
    const int Q = (int)qs.size();
    *out = Cands();
    if (Q == 0) return ORBX_OK;
    Packer pq(h, h->h_packB, SR_QUERY);
    const size_t pqs = pq.add(qs.data(), sizeof(AreaQuery) * (size_t)Q), pqd = pq.add(qdesc, 32 * (size_t)Q);
    if (int e = pq.flush()) return fail(ORBX_E_DEVICE, "%s", upload_error(e));
    return pooled_area_search(h, Q, 0, "area search", [&](const AreaBlock& o, size_t pool) {
        rt::memset_async(o.counter, 0, 16, h->s0);
        launch_area_search(h, D, Q, pq.dev<AreaQuery>(pqs), pq.dev<unsigned long long>(pqd), o, pool);
    }, out);
}

}  // namespace

extern "C" {

int orbm_get_features_in_area(orbx_extractor* h, const OrbmFrameView* F, float x, float y, float r, int min_level, int max_level, int* indices, int cap) {
    if (!h || !indices) return fail(ORBX_E_ARG, "null");
    rt::set_device(h->device);
    DeviceFrame D;
    int rc = upload_frame(h, F, &D); if (rc) return rc;
    std::vector<AreaQuery> qs(1);
    qs[0].x = x; qs[0].y = y; qs[0].r = r; qs[0].ur = 0; qs[0].min_level = min_level; qs[0].max_level = max_level; qs[0].active = 1; qs[0].gate = 0;
    uint8_t zero[32] = {0};
    Cands c;
    rc = run_area_search(h, D, qs, zero, &c); if (rc) return rc;
    for (int k = 0; k < c.count[0] && k < cap; k++) indices[k] = c.idx(0, k);
    return c.count[0];
}

int orbm_area_search_batch(orbx_extractor* h, const OrbmFrameView* F, const OrbmAreaQuery* queries, const uint8_t* query_desc, int Q,
                           int* start, int* count, int* idx, int* dist, int* level, int cap) {
    if (!h || !F || (Q > 0 && (!queries || !query_desc || !start || !count))) return fail(ORBX_E_ARG, "null");
    rt::set_device(h->device);
    DeviceFrame D;
    int rc = upload_frame(h, F, &D); if (rc) return rc;
    std::vector<AreaQuery> qs(Q);
    for (int i = 0; i < Q; i++) {
        AreaQuery& q = qs[i]; memset(&q, 0, sizeof q);
        q.x = queries[i].x; q.y = queries[i].y; q.r = queries[i].r; q.min_level = queries[i].min_level; q.max_level = queries[i].max_level;
        q.active = 1; q.gate = 0;
    }
    Cands c;
    rc = run_area_search(h, D, qs, query_desc, &c); if (rc) return rc;
    int total = 0;
    for (int i = 0; i < Q; i++) { start[i] = c.start[i]; count[i] = c.count[i]; total = std::max(total, c.start[i] + c.count[i]); }
    if (total <= cap && idx && dist && level)               // (the queries' spans tile the pool: every entry belongs to one of them)
        for (int i = 0; i < Q; i++)
            for (int k = 0; k < c.count[i]; k++) { const int e = c.start[i] + k; idx[e] = c.idx(i, k); dist[e] = c.dist(i, k); level[e] = c.level(i, k); }
    return total;
}

int orbm_search_by_projection_mappoints(orbx_extractor* h, const OrbmFrameView* F, const OrbmMapPointView* P, float th, int far_points,
                                        float th_far, float nnratio, int* assigned, int* nmatches_out) {
    if (!h || !F || !P || !assigned) return fail(ORBX_E_ARG, "null");
    rt::set_device(h->device);
    DeviceFrame D;
    int rc = upload_frame(h, F, &D); if (rc) return rc;
    const int M = P->M, N = F->N;
    const bool bFactor = th != 1.0;
    std::vector<AreaQuery> qs(M);
    for (int i = 0; i < M; i++) {
        AreaQuery& q = qs[i]; memset(&q, 0, sizeof q);
        // :53-60 skip tests; (the right-camera branch :170-236 needs Nleft != -1 and is not part of this path)
        if (!P->in_view[i]) continue;
        if (far_points && P->track_depth[i] > th_far) continue;
        if (P->is_bad[i]) continue;
        const int lvl = P->scale_level[i];
        if (lvl < 0 || lvl >= F->nlevels) continue;
        float r = P->view_cos[i] > 0.998 ? 2.5f : 4.0f;                 // RadiusByViewingCos, :242-249
        if (bFactor) r *= th;
        q.x = P->proj_x[i]; q.y = P->proj_y[i]; q.r = r * F->scale_factors[lvl]; q.ur = P->proj_xr[i];
        q.min_level = lvl - 1; q.max_level = lvl; q.active = 1; q.gate = 1;
    }
    Cands c;
    rc = run_area_search(h, D, qs, P->desc, &c); if (rc) return rc;
    std::vector<uint8_t> occ(N > 0 ? N : 1, 0);
    if (F->occupied) memcpy(occ.data(), F->occupied, N);
    for (int i = 0; i < N; i++) assigned[i] = -1;
    const int nmatches = replay_mappoints(c, M, nnratio, P->has_obs, occ.data(), assigned);      // (an inactive query has no candidates)
    if (nmatches_out) *nmatches_out = nmatches;
    return ORBX_OK;
}

// ---- C1 on the device: Frame::isInFrustum + MapPoint::PredictScale (k_frustum), alone or in front of SearchByProjection(Frame, MapPoints) ----
namespace {
struct FrustumDev { uint8_t* in_view; float* track; int* level; AreaQuery* queries; const unsigned long long* qdesc; };
// what k_frustum writes for M points, one block per camera: [track 5 M][level M][in_view M]
struct TrackBlock {
    size_t level, in_view, bytes;
    explicit TrackBlock(int M) { Bump b; b.take(20 * (size_t)std::max(M, 1)); level = b.take(4 * (size_t)std::max(M, 1)); in_view = b.take((size_t)std::max(M, 1)); bytes = b.o; }
};
void launch_frustum(orbx_extractor* h, const FrustumParams& F, int M, const float* pos, const float* normal, const float* min_d, const float* max_d, const uint8_t* bad,
                    uint8_t* track, AreaQuery* queries, int* counter) {
    const TrackBlock T(M);
    dim3 grid((M + 255) / 256, 1, 1), blk(256, 1, 1);
    ORBX_LAUNCH(k_frustum, grid, blk, 0, h->s0, F, M, pos, normal, min_d, max_d, bad, track + T.in_view, (float*)track, (int*)(track + T.level), queries, counter);
}
int enqueue_frustum(orbx_extractor* h, const OrbmFrustumView* V, const OrbmWorldPointView* P, float cos_limit, bool with_queries, float th, int far_points, float th_far,
                    FrustumDev* out, const FrustumParams* second = nullptr, FrustumDev* out2 = nullptr) {
    if (!V || !P || P->M < 0 || (P->M > 0 && (!P->pos || !P->normal || !P->min_distance || !P->max_distance))) return fail(ORBX_E_ARG, "bad frustum arguments");
    if (V->nlevels < 1 || V->nlevels > kMaxLevels || !V->scale_factors) return fail(ORBX_E_ARG, "bad scale levels");
    const int M = P->M; const size_t M1 = M > 0 ? M : 1, Mn = M;
    if (M > 0 && !P->desc && with_queries) return fail(ORBX_E_ARG, "map point descriptors missing");
    // inputs -> d_sr[SR_QUERY]: [descriptors][pos][normal][min][max][bad], the queries behind them; outputs -> d_sr[SR_SPARE]: one TrackBlock per camera
    Packer pk(h, h->h_packB, SR_QUERY);
    const size_t pd = pk.add(P->desc, P->desc ? 32 * Mn : 0), pp = pk.add(P->pos, 12 * Mn), pn = pk.add(P->normal, 12 * Mn), pmn = pk.add(P->min_distance, 4 * Mn),
                 pmx = pk.add(P->max_distance, 4 * Mn), pb = P->is_bad ? pk.add(P->is_bad, Mn) : pk.fill(0, Mn), pq = pk.room(sizeof(AreaQuery) * M1);
    const TrackBlock T(M);
    if (h->d_sr[SR_SPARE].ensure(2 * T.bytes + 16)) return fail(ORBX_E_DEVICE, "upload/allocation failed");
    if (int e = pk.flush()) return fail(ORBX_E_DEVICE, "%s", upload_error(e));
    FrustumParams F; fill_frustum_params(V, cos_limit, th, far_points, th_far, &F);     // (k_frustum does not read qcw)
    F.rig_mode = second ? 1 : 0;
    uint8_t* dout = h->d_sr[SR_SPARE].p;
    out->in_view = dout + T.in_view; out->track = (float*)dout; out->level = (int*)(dout + T.level);
    out->queries = with_queries ? pk.out<AreaQuery>(pq) : nullptr; out->qdesc = pk.dev<unsigned long long>(pd);
    if (M > 0) launch_frustum(h, F, M, pk.dev<float>(pp), pk.dev<float>(pn), pk.dev<float>(pmn), pk.dev<float>(pmx), pk.dev<uint8_t>(pb), dout, out->queries, nullptr);
    if (second && out2) {                                           // the second camera of a rig: the same points, its own block behind the first one
        uint8_t* dout2 = dout + T.bytes;                            // (both cameras of a rig store nothing for a rejected point; the caller passed V with rig semantics)
        out2->in_view = dout2 + T.in_view; out2->track = (float*)dout2; out2->level = (int*)(dout2 + T.level); out2->queries = nullptr; out2->qdesc = out->qdesc;
        if (M > 0) launch_frustum(h, *second, M, pk.dev<float>(pp), pk.dev<float>(pn), pk.dev<float>(pmn), pk.dev<float>(pmx), pk.dev<uint8_t>(pb), dout2, nullptr, nullptr);
    }
    return ORBX_OK;
}
// hands the tracking fields (host copy of one TrackBlock) to the caller's arrays
void scatter_track(const uint8_t* blk, int M, const OrbmTrackOut* out) {
    if (!out || M <= 0) return;
    const TrackBlock T(M);
    const size_t M1 = M;
    const float* tr = (const float*)blk;
    if (out->in_view) memcpy(out->in_view, blk + T.in_view, M1);
    if (out->proj_x) memcpy(out->proj_x, tr, 4 * M1);
    if (out->proj_y) memcpy(out->proj_y, tr + M1, 4 * M1);
    if (out->proj_xr) memcpy(out->proj_xr, tr + 2 * M1, 4 * M1);
    if (out->depth) memcpy(out->depth, tr + 3 * M1, 4 * M1);
    if (out->view_cos) memcpy(out->view_cos, tr + 4 * M1, 4 * M1);
    if (out->scale_level) memcpy(out->scale_level, blk + T.level, 4 * M1);
}
// brings the block back (one copy into pinned memory) and scatters it
int fetch_frustum(orbx_extractor* h, int M, const FrustumDev& D, const OrbmTrackOut* out) {
    if (M <= 0) return ORBX_OK;
    const size_t n = TrackBlock(M).bytes;
    if (h->h_out.ensure(n + 16)) return fail(ORBX_E_DEVICE, "pinned allocation failed");
    if (rt::copy_d2h(h->h_out.p, D.track, n, h->s0) || rt::stream_sync(h->s0) || rt::check_launch()) return fail(ORBX_E_DEVICE, "frustum kernel failed: %s", rt::last_error());
    scatter_track(h->h_out.p, M, out);
    return ORBX_OK;
}
}  // namespace

int orbm_is_in_frustum(orbx_extractor* h, const OrbmFrustumView* V, const OrbmWorldPointView* P, float cos_limit, const OrbmTrackOut* out) {
    if (!h || !out) return fail(ORBX_E_ARG, "null");
    rt::set_device(h->device);
    FrustumDev D;
    int rc = enqueue_frustum(h, V, P, cos_limit, false, 1.0f, 0, 0.0f, &D); if (rc) return rc;
    return fetch_frustum(h, P->M, D, out);
}

// ---- Frame::isInFrustum with two cameras (Nleft != -1, src/Frame.cc:754-766): isInFrustumChecks (:1592-1650) once per camera ----
namespace {
// a coefficient of an Eigen (>= 3.3) 3x3 product: a0 b0 + (a1 b1 + a2 b2) (sophus_action.h)
inline float dot3(const float* a, int sa, const float* b, int sb) { return a[0] * b[0] + (a[sa] * b[sb] + a[2 * sa] * b[2 * sb]); }
// camera 2 of the rig as isInFrustumChecks(pMP, cos, bRight = true) sets it up: mR = Rrl * mRcw, mt = Rrl * mtcw + trl, twc = mRwc * tlr + mOw
void right_camera_params(const OrbmFrustumRigView* V, float cos_limit, FrustumParams* Fp) {
    OrbmFrustumView R = V->left;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R.Rcw[3 * i + j] = dot3(V->Rrl + 3 * i, 1, V->left.Rcw + j, 3);
    for (int i = 0; i < 3; i++) R.tcw[i] = dot3(V->Rrl + 3 * i, 1, V->left.tcw, 1) + V->trl[i];
    for (int i = 0; i < 3; i++) R.Ow[i] = dot3(V->Rwc + 3 * i, 1, V->tlr, 1) + V->left.Ow[i];
    R.camera_type = V->camera2_type; memcpy(R.cam, V->cam2, sizeof R.cam);
    fill_frustum_params(&R, cos_limit, 1.0f, 0, 0.0f, Fp);
    Fp->rig_mode = 1;
}
void scatter_track_right(const uint8_t* blk, int M, const OrbmTrackOutRight* out) {
    if (!out || M <= 0) return;
    const TrackBlock T(M);
    const size_t M1 = M;
    const float* tr = (const float*)blk;
    if (out->in_view_r) memcpy(out->in_view_r, blk + T.in_view, M1);
    if (out->proj_xr) memcpy(out->proj_xr, tr, 4 * M1);
    if (out->proj_yr) memcpy(out->proj_yr, tr + M1, 4 * M1);
    if (out->depth_r) memcpy(out->depth_r, tr + 3 * M1, 4 * M1);
    if (out->view_cos_r) memcpy(out->view_cos_r, tr + 4 * M1, 4 * M1);
    if (out->scale_level_r) memcpy(out->scale_level_r, blk + T.level, 4 * M1);
}
}  // namespace

int orbm_is_in_frustum_rig(orbx_extractor* h, const OrbmFrustumRigView* V, const OrbmWorldPointView* P, float cos_limit, const OrbmTrackOut* left, const OrbmTrackOutRight* right) {
    if (!h || !V || !P || !left || !right) return fail(ORBX_E_ARG, "null");
    rt::set_device(h->device);
    FrustumParams Fr; right_camera_params(V, cos_limit, &Fr);
    FrustumDev D, D2;
    int rc = enqueue_frustum(h, &V->left, P, cos_limit, false, 1.0f, 0, 0.0f, &D, &Fr, &D2); if (rc) return rc;
    const int M = P->M;
    if (M <= 0) return ORBX_OK;
    const size_t n = TrackBlock(M).bytes;
    if (h->h_out.ensure(2 * n + 16)) return fail(ORBX_E_DEVICE, "pinned allocation failed");
    if (rt::copy_d2h(h->h_out.p, D.track, 2 * n, h->s0) || rt::stream_sync(h->s0) || rt::check_launch()) return fail(ORBX_E_DEVICE, "frustum kernel failed: %s", rt::last_error());
    scatter_track(h->h_out.p, M, left);
    scatter_track_right(h->h_out.p + n, M, right);
    return ORBX_OK;
}

// ---- map points that stay on the device (the local map changes slowly; Tracking::SearchLocalPoints visits it every frame) ----
struct orbm_points {
    int device = 0, M = 0;
    uint8_t* dmem = nullptr;
    const unsigned long long* desc = nullptr; const float *pos = nullptr, *normal = nullptr, *min_d = nullptr, *max_d = nullptr;
    bool map_owned = false;      // a set an orbm_map built: its memory is the map's
};

int orbm_points_create(orbx_extractor* h, const OrbmWorldPointView* P, orbm_points** out) {
    if (!h || !P || !out || P->M < 0 || (P->M > 0 && (!P->pos || !P->normal || !P->min_distance || !P->max_distance || !P->desc))) return fail(ORBX_E_ARG, "bad map point view");
    rt::set_device(h->device);
    const size_t M1 = P->M > 0 ? P->M : 1;
    const size_t od = 0, op = od + al16(32 * M1), on = op + al16(12 * M1), omn = on + al16(12 * M1), omx = omn + al16(4 * M1), total = omx + al16(4 * M1);
    std::vector<uint8_t> st(total, 0);
    if (P->M > 0) {
        memcpy(&st[od], P->desc, 32 * (size_t)P->M); memcpy(&st[op], P->pos, 12 * (size_t)P->M); memcpy(&st[on], P->normal, 12 * (size_t)P->M);
        memcpy(&st[omn], P->min_distance, 4 * (size_t)P->M); memcpy(&st[omx], P->max_distance, 4 * (size_t)P->M);
    }
    orbm_points* r = new orbm_points();
    r->device = h->device; r->M = P->M; r->dmem = (uint8_t*)rt::dmalloc(total);
    if (!r->dmem || rt::copy_h2d(r->dmem, st.data(), total, h->s0) || rt::stream_sync(h->s0)) { rt::dfree(r->dmem); delete r; return fail(ORBX_E_DEVICE, "map point upload failed"); }
    r->desc = (const unsigned long long*)(r->dmem + od); r->pos = (const float*)(r->dmem + op); r->normal = (const float*)(r->dmem + on);
    r->min_d = (const float*)(r->dmem + omn); r->max_d = (const float*)(r->dmem + omx);
    *out = r;
    return ORBX_OK;
}

void orbm_points_destroy(orbm_points* p) {
    if (!p || p->map_owned) return;
    rt::set_device(p->device);
    rt::dfree(p->dmem);
    delete p;
}

namespace {
// Tracking::SearchLocalPoints' device part (src/Tracking.cc:4009-4067): Frame::isInFrustum for every candidate map point, then
// ORBmatcher::SearchByProjection(Frame, MapPoints, th, bFarPoints, thFarPoints) on the points in view.  One upload (the frame, the call-time
// flags and - unless the points are resident - the points), three launches (grid, frustum + window queries, window search), one download
// (tracking fields, candidate lists), then the ordered replay of src/ORBmatcher.cc:62-166 on the host.
int search_local_points_core(orbx_extractor* h, const OrbmFrameView* F, const OrbmFrustumView* V, int M, const OrbmWorldPointView* P, const orbm_points* R,
                             const uint8_t* is_bad, const uint8_t* has_obs, float cos_limit, float th, int far_points, float th_far, float nnratio,
                             const OrbmTrackOut* out, int* assigned, int* nmatches_out) {
    int rc = frame_check(F); if (rc) return rc;
    if (!V || V->nlevels < 1 || V->nlevels > kMaxLevels || !V->scale_factors) return fail(ORBX_E_ARG, "bad scale levels");
    const int N = F->N;
    for (int i = 0; i < N; i++) assigned[i] = -1;
    if (nmatches_out) *nmatches_out = 0;
    if (M <= 0) return ORBX_OK;
    const size_t M1 = M;
    if (h->d_sr[SR_QUERY].ensure(sizeof(AreaQuery) * M1 + 16)) return fail(ORBX_E_DEVICE, "upload/allocation failed");
    // input block: frame [keys | descriptors | uRight] | bad flags | (host points: descriptors | pos | normal | min | max)
    Packer pk(h);
    size_t pb = 0, pd = 0, pp = 0, pn = 0, pmn = 0, pmx = 0;
    DeviceFrame D;
    rc = upload_frame(h, F, &D, pk, [&] {
        pb = is_bad ? pk.add(is_bad, M1) : pk.fill(0, M1);
        if (!R) { pd = pk.add(P->desc, 32 * M1); pp = pk.add(P->pos, 12 * M1); pn = pk.add(P->normal, 12 * M1); pmn = pk.add(P->min_distance, 4 * M1); pmx = pk.add(P->max_distance, 4 * M1); }
    });
    if (rc) return rc;
    FrustumParams Fp; fill_frustum_params(V, cos_limit, th, far_points, th_far, &Fp);     // (k_frustum does not read qcw)
    AreaQuery* dq = (AreaQuery*)h->d_sr[SR_QUERY].p;
    const unsigned long long* dqd = R ? R->desc : pk.dev<unsigned long long>(pd);
    // output block: [counter 16 | start M | count M] | tracking fields | candidate entries
    Cands c; const uint8_t* track = nullptr;
    rc = pooled_area_search(h, M, TrackBlock(M).bytes, "local point search", [&](const AreaBlock& o, size_t pool) {
        launch_frustum(h, Fp, M, R ? R->pos : pk.dev<float>(pp), R ? R->normal : pk.dev<float>(pn), R ? R->min_d : pk.dev<float>(pmn), R ? R->max_d : pk.dev<float>(pmx),
                       pk.dev<uint8_t>(pb), o.mid, dq, o.counter);
        launch_area_search(h, D, M, dq, dqd, o, pool);
    }, &c, &track);
    if (rc) return rc;
    scatter_track(track, M, out);
    std::vector<uint8_t> occ(N > 0 ? N : 1, 0);
    if (F->occupied) memcpy(occ.data(), F->occupied, N);
    const int nmatches = replay_mappoints(c, M, nnratio, has_obs, occ.data(), assigned);
    if (nmatches_out) *nmatches_out = nmatches;
    return ORBX_OK;
}
}  // namespace

int orbm_search_local_points(orbx_extractor* h, const OrbmFrameView* F, const OrbmFrustumView* V, const OrbmWorldPointView* P, float cos_limit, float th,
                             int far_points, float th_far, float nnratio, const OrbmTrackOut* out, int* assigned, int* nmatches_out) {
    if (!h || !F || !V || !P || !assigned) return fail(ORBX_E_ARG, "null");
    if (P->M < 0 || (P->M > 0 && (!P->pos || !P->normal || !P->min_distance || !P->max_distance || !P->desc))) return fail(ORBX_E_ARG, "bad map point view");
    rt::set_device(h->device);
    return search_local_points_core(h, F, V, P->M, P, nullptr, P->is_bad, P->has_obs, cos_limit, th, far_points, th_far, nnratio, out, assigned, nmatches_out);
}

int orbm_search_local_points_resident(orbx_extractor* h, const OrbmFrameView* F, const OrbmFrustumView* V, const orbm_points* points, const uint8_t* is_bad,
                                      const uint8_t* has_obs, float cos_limit, float th, int far_points, float th_far, float nnratio, const OrbmTrackOut* out,
                                      int* assigned, int* nmatches_out) {
    if (!h || !F || !V || !points || !assigned) return fail(ORBX_E_ARG, "null");
    if (points->device != h->device) return fail(ORBX_E_ARG, "map points live on another device");
    rt::set_device(h->device);
    return search_local_points_core(h, F, V, points->M, nullptr, points, is_bad, has_obs, cos_limit, th, far_points, th_far, nnratio, out, assigned, nmatches_out);
}

// ---- the batched, device-resident form of Tracking::SearchLocalPoints ----------------------------------------------
// Frames = images [first, first + B) of the handle's last extraction, read where the extractor left them (keypoints, descriptors, counts; uRight
// from orbm_stereo_match / orbm_stereo_from_depth); map points resident (orbm_points); one pose per frame.  Five launches for the whole batch:
// grid build (B workgroups), frustum + window queries (B x M threads), window search (B x M waves), accept loop (one wave per frame) - nothing
// visits the host between them; one upload (poses + call-time flags), one download (assignments, match counts, optionally mbTrackInView).

int orbm_stereo_from_depth(orbx_extractor* h, int first, int B, const float* depth, int stride, size_t image_stride, int on_device, float mbf) {
    if (!h || !depth || B <= 0 || first < 0 || first + B > h->lastB) return fail(ORBX_E_ARG, "bad frame range");
    if (stride < h->W || (B > 1 && image_stride < (size_t)stride * (h->H - 1) + h->W)) return fail(ORBX_E_ARG, "depth stride too small");
    if (undistort_stale(h)) return fail(ORBX_E_ARG, "orbx_set_undistort was called after the last extraction: extract again before orbm_stereo_from_depth");
    rt::set_device(h->device);
    const float* d_depth = depth;
    if (!on_device) {
        const size_t n = (size_t)(B - 1) * image_stride + (size_t)stride * (h->H - 1) + h->W;
        if (h->d_depth_in.ensure(n * sizeof(float) + 16) || rt::copy_h2d(h->d_depth_in.p, depth, n * sizeof(float), h->s0)) return fail(ORBX_E_DEVICE, "depth upload failed");
        d_depth = (const float*)h->d_depth_in.p;
    }
    const int cap = h->kp_total_cap;
    rt::memset_async(h->d_nmatch.p, 0, sizeof(int) * (size_t)B, h->s0);
    dim3 grid((cap + 255) / 256, B, 1), blk(256, 1, 1);
    ORBX_LAUNCH(k_stereo_from_depth, grid, blk, 0, h->s0, (const KeyPointRec*)(h->d_kps.p + (size_t)first * cap),
                h->ex_undist_active ? (const KeyPointRec*)(h->d_kps_un.p + (size_t)first * cap) : (const KeyPointRec*)nullptr, (const int*)(h->d_nm.p + first), cap,
                d_depth, stride, image_stride, h->W, h->H, mbf, h->d_uRight.p, h->d_depth.p, h->d_nmatch.p);
    h->ur_B = 0;
    if (rt::check_launch()) return fail(ORBX_E_DEVICE, "kernel launch failed: %s", rt::last_error());
    h->ur_first = first; h->ur_B = B; h->ur_gen = h->extract_gen; h->depth_is_rig = false;
    return ORBX_OK;
}

}  // extern "C"
namespace {
// ---- pieces that the batched routes (one camera and rig) share ----
// the poses of a batch, `stride` bytes apart (a rig batch passes &f[0].left): scale levels, and one grid geometry per batch
int frames_check(const OrbmFrustumView* f0, size_t stride, int B) {
    for (int b = 0; b < B; b++) {
        const OrbmFrustumView& v = *(const OrbmFrustumView*)((const uint8_t*)f0 + (size_t)b * stride);
        if (v.nlevels < 1 || v.nlevels > kMaxLevels || !v.scale_factors) return fail(ORBX_E_ARG, "bad scale levels (frame %d)", b);
        // (the frames of a batch come from one extraction: one image size)
        if (v.min_x != f0->min_x || v.max_x != f0->max_x || v.min_y != f0->min_y || v.max_y != f0->max_y) return fail(ORBX_E_ARG, "frame %d has other image bounds than frame 0", b);
    }
    if (!(f0->max_x > f0->min_x) || !(f0->max_y > f0->min_y)) return fail(ORBX_E_ARG, "empty image bounds");
    return ORBX_OK;
}
GridParams grid_from_view(const OrbmFrustumView& v) {
    GridParams g; memset(&g, 0, sizeof g);
    g.min_x = v.min_x; g.min_y = v.min_y;
    g.gw_inv = (float)kGridColsHost / (v.max_x - v.min_x); g.gh_inv = (float)kGridRowsHost / (v.max_y - v.min_y);   // src/Frame.cc:190-191
    return g;
}
// entries of the candidate pool: what the last batch grew it to, or `expected` for this one; the kernels count entries in an int
size_t batch_pool(const orbx_extractor* h, size_t expected) { return std::min<size_t>(std::max(h->lp_pool, expected), 0x7fffffff / 2); }
// The local maps of a batched SearchLocalPoints, staged as the table the kernels read (FrameMapRec, orbx_types.h): ONE resident set and one pair of flag
// arrays for every frame (maps == nullptr: the set B times, frame b's scratch rows at b * M, the flags uploaded once), or one OrbmFrameMap per frame
// (frame b's rows and flags at the prefix sum of M_b), or the sets of an orbm_map where its builds left them (sets[b]: the record of frame b's set with the M
// it holds now; laid out as `maps`, but the flags are not staged: k_map_set_flags writes them on the device from the table flag_table() fills)
struct BatchMaps {
    const orbm_points* one; const uint8_t *is_bad, *has_obs; const OrbmFrameMap* maps; int B;
    const MapSetRec* sets = nullptr;
    int m_max = 0; size_t rows = 1, flags = 1;     // largest map; scratch rows of the batch; bytes of ONE uploaded flag array
    std::vector<int> M;                            // per frame
    size_t table_bytes() const { return sizeof(FrameMapRec) * (size_t)B; }
    const orbm_points* set(int b) const { return maps ? maps[b].points : one; }
    int plan(int device) {
        if (!maps && !sets && one->device != device) return fail(ORBX_E_ARG, "map points live on another device");
        size_t sum = 0;
        M.resize(B);
        for (int b = 0; b < B; b++) {
            const orbm_points* s = sets ? nullptr : set(b);
            if (s && s->device != device) return fail(ORBX_E_ARG, "frame %d: its map points live on another device", b);
            M[b] = sets ? std::max(sets[b].M, 0) : (s && s->M > 0 ? s->M : 0);
            sum += (size_t)M[b]; m_max = std::max(m_max, M[b]);
        }
        if (sum > 0x7fffffff / 32) return fail(ORBX_E_CAPACITY, "%zu map points in one batch", sum);      // (offsets are ints; 5 floats of track per row)
        rows = sum > 0 ? sum : 1;
        flags = (maps || sets) ? rows : (size_t)std::max(m_max, 1);
        return ORBX_OK;
    }
    static void stage_flags(uint8_t* bad, uint8_t* obs, const uint8_t* is_bad, const uint8_t* has_obs, size_t m) {
        if (is_bad) memcpy(bad, is_bad, m); else memset(bad, 0, m);
        if (has_obs) memcpy(obs, has_obs, m); else memset(obs, 1, m);
    }
    void stage(uint8_t* tab, uint8_t* bad, uint8_t* obs) const {
        FrameMapRec* T = (FrameMapRec*)tab;
        size_t o = 0;
        for (int b = 0; b < B; b++) {
            const size_t m = (size_t)M[b];
            FrameMapRec r; memset(&r, 0, sizeof r);
            if (m && sets) { const MapSetRec& s = sets[b]; r.pos = s.pos; r.normal = s.normal; r.min_d = s.min_d; r.max_d = s.max_d; r.desc = s.desc; }
            else if (m) { const orbm_points* s = set(b); r.pos = s->pos; r.normal = s->normal; r.min_d = s->min_d; r.max_d = s->max_d; r.desc = s->desc; }
            r.M = (int)m; r.offset = (int)o; r.flags = (maps || sets) ? (int)o : 0;
            T[b] = r;
            if (maps) stage_flags(bad + o, obs + o, maps[b].is_bad, maps[b].has_obs, m);
            o += m;
        }
        if (!maps && !sets) stage_flags(bad, obs, is_bad, has_obs, (size_t)m_max);
    }
    // the sets form: what k_map_set_flags and k_assigned_slots read of frame b's set
    size_t flag_table_bytes() const { return sets ? sizeof(SetFlagRec) * (size_t)B : 0; }
    void flag_table(uint8_t* tab) const {
        SetFlagRec* T = (SetFlagRec*)tab;
        size_t o = 0;
        for (int b = 0; b < B; b++) { T[b] = {M[b] ? sets[b].seen : nullptr, M[b] ? sets[b].slots : nullptr, M[b], (int)o}; o += (size_t)M[b]; }
    }
    // the flags of the sets form, written behind the upload on the batch's stream
    void gather_flags(rt::stream_t s, const uint8_t* d_tab, uint8_t* d_bad, uint8_t* d_obs) const {
        if (m_max <= 0) return;
        const dim3 grid((unsigned)std::max<size_t>(1, ((size_t)m_max / 4 + 255) / 256), B, 1), blk(256, 1, 1);      // (a dword per thread; block 0 also copies the ragged ends)
        ORBX_LAUNCH(k_map_set_flags, grid, blk, 0, s, (const SetFlagRec*)d_tab, d_bad, d_obs);
    }
    void translate(rt::stream_t s, const uint8_t* d_tab, const int* d_assigned, int S, int* d_out) const {
        const dim3 grid((unsigned)((S + 255) / 256), B, 1), blk(256, 1, 1);
        ORBX_LAUNCH(k_assigned_slots, grid, blk, 0, s, (const SetFlagRec*)d_tab, d_assigned, S, d_out);
    }
};
// the table of a projection batch (LastFrame / KeyFrame points): frame b's M rows of the uploaded descriptors (d_desc: their device address), everything at b * M
void stage_uniform_table(uint8_t* tab, int B, int M, const unsigned long long* d_desc) {
    FrameMapRec* T = (FrameMapRec*)tab;
    for (int b = 0; b < B; b++) {
        FrameMapRec r; memset(&r, 0, sizeof r);
        r.desc = d_desc + 4 * (size_t)b * (size_t)M; r.M = M; r.offset = r.flags = b * M;
        T[b] = r;
    }
}
// the grid of one camera for B frames (k_grid_build: cell_of, cell_start, cell_items)
struct GridBlock {
    size_t cof, cst, cit;
    GridBlock(Bump& d, size_t B1, size_t C1) { cof = d.take(4 * B1 * C1); cst = d.take(4 * B1 * kGridCellStride); cit = d.take(4 * B1 * C1); }
};
// the result of a batch, [counter 16 | nmatches B | assigned B x slots | a batch on a map's own sets: assigned as map slots, B x slots]: laid out by the
// enqueue, read back by the fetch in one copy
struct ResultBlock {
    size_t nmatches, assigned, as_slots, bytes;
    ResultBlock(size_t B1, size_t slots, bool slot_result = false)
        : nmatches(16), assigned(16 + al16(4 * B1)), as_slots(assigned + (slot_result ? 4 * B1 * slots : 0)), bytes(as_slots + 4 * B1 * slots) {}
};

// ---- the frame of a batched enqueue.  Each of the four (local_points_batch, projection_batch, local_points_rig_batch, lastframe_rig_batch) keeps what is its
// own - the checks of its arguments, its LDS formula, the rows it uploads, its query launch and its accept launch - around these steps, in this order:
//   batch_clear      the first line of every entry point: a new enqueue - accepted or refused - ends the previous batch, so a refused call leaves nothing to fetch
//   every refusal    BEFORE anything is enqueued into the shared block
//   batch_reserve    waits for the staging block of the previous enqueue, makes room for this one
//   batch_upload     the staging block goes up (map-fed rows: and are gathered); ev_lp is recorded behind it
//   camera_searches / rig_searches     grids, the caller's query launch, the window searches into the entry pool
//   batch_finish     behind the caller's accept launch: the record of the pending batch is assigned, whole
void batch_clear(orbx_extractor* h) { if (h) h->batch = PendingBatch(); }
// room for the device block (`pool` candidate entries behind o_pool), u_total bytes of staging and out_bytes of results; false: an allocation failed
bool batch_reserve(orbx_extractor* h, size_t o_pool, size_t pool, size_t u_total, size_t out_bytes) {
    if (h->lp_pending) rt::event_sync(h->ev_lp);                // the staging block of the previous enqueue has been consumed
    if (h->d_lp.ensure(o_pool + pool * 8 + 64) || h->h_lp_in.ensure(u_total + 16) || h->h_lp_out.ensure(out_bytes + 64)) return false;
    h->lp_pool = pool;
    return true;
}
int batch_finish(orbx_extractor* h, const PendingBatch& enqueued) {
    if (h->profile) rt::event_record(h->ev_stage[ST_MATCH][1], h->s0);
    if (rt::check_launch()) return fail(ORBX_E_DEVICE, "kernel launch failed: %s", rt::last_error());
    h->batch = enqueued;
    return ORBX_OK;
}
// one record per frame of map points seen from somewhere else: the LastFrame's (octave of its keypoint, has_obs) or a key frame's (distance limits)
struct PointRows {
    int cap; const int* n; const float* pos; const uint8_t* valid; const int* octave; const float* angle; const uint8_t* has_obs; const uint8_t* desc;
    const float* min_distance; const float* max_distance;          // key-frame form only
};
PointRows last_frame_rows(const OrbmLastFrameBatch* last) {
    return {last->cap_last, last->n, last->pos, last->valid, last->octave, last->angle, last->has_obs, last->desc, nullptr, nullptr};
}
// The same rows named by their place in an orbm_map (the .._batch_map calls): the fields come from the store, gathered on the device.  Last frame: slots
// [B][cap] (LastFrame.mvpMapPoints), the PointRows carries n, octave, angle and has_obs.  Key frame: recs[b] = the key frame's row of slots and its resident
// keypoints (device addresses), the PointRows carries n = the rows' lengths.  excluded: mvbOutlier / sAlreadyFound, rows `excluded_stride` apart (nullptr = none)
struct MapRows { MapStore S; const int* slots; const MapRowRec* recs; const uint8_t* excluded; size_t excluded_stride; };
// their place in the device block and the copy into the staging buffer.  Host-fed rows go up whole: n_last | pos | valid | octave | angle | has_obs |
// descriptors.  Map-fed rows (src): n_last | excluded | has_obs | slots, octave, angle (last frame) or the row records (key frame) go up, and
// device_rows() lays pos, valid, descriptors and a key frame's distance limits and angles out BEHIND the upload, where gather() writes them
struct PointRowsUpload {
    size_t u_n, u_pos = 0, u_val = 0, u_oct = 0, u_ang = 0, u_obs, u_desc = 0, u_mxd = 0, u_exc = 0, u_src = 0;
    const MapRows* src; bool keyframe;
    PointRowsUpload(Bump& u, size_t B1, size_t M1, const MapRows* from_map = nullptr, bool kf = false) : src(from_map), keyframe(kf) {
        u_n = u.take(4 * B1);
        if (!src) {
            u_pos = u.take(12 * B1 * M1); u_val = u.take(B1 * M1); u_oct = u.take(4 * B1 * M1); u_ang = u.take(4 * B1 * M1); u_obs = u.take(B1 * M1);
            u_desc = u.take(32 * B1 * M1);
            return;
        }
        u_exc = u.take(B1 * M1); u_obs = u.take(B1 * M1);
        if (keyframe) u_src = u.take(sizeof(MapRowRec) * B1);
        else { u_src = u.take(4 * B1 * M1); u_oct = u.take(4 * B1 * M1); u_ang = u.take(4 * B1 * M1); }
    }
    void device_rows(Bump& d, size_t B1, size_t M1) {
        if (!src) return;
        u_pos = d.take(12 * B1 * M1); u_val = d.take(B1 * M1); u_desc = d.take(32 * B1 * M1);
        if (keyframe) { u_oct = d.take(4 * B1 * M1); u_mxd = d.take(4 * B1 * M1); u_ang = d.take(4 * B1 * M1); }
    }
    void stage(uint8_t* hp, const PointRows& last, size_t B1, size_t M1) const {
        memcpy(hp + u_n, last.n, 4 * B1);
        if (last.has_obs) memcpy(hp + u_obs, last.has_obs, B1 * M1); else memset(hp + u_obs, 1, B1 * M1);
        if (!src) {
            memcpy(hp + u_pos, last.pos, 12 * B1 * M1); memcpy(hp + u_val, last.valid, B1 * M1);
            if (last.octave) memcpy(hp + u_oct, last.octave, 4 * B1 * M1); else memcpy(hp + u_oct, last.min_distance, 4 * B1 * M1);      // (a key frame's octave rows carry mfMinDistance)
            memcpy(hp + u_ang, last.angle, 4 * B1 * M1);
            memcpy(hp + u_desc, last.desc, 32 * B1 * M1);
            return;
        }
        memset(hp + u_exc, 0, B1 * M1);
        if (src->excluded) for (size_t b = 0; b < B1; b++) memcpy(hp + u_exc + b * M1, src->excluded + b * src->excluded_stride, (size_t)last.n[b]);
        if (keyframe) memcpy(hp + u_src, src->recs, sizeof(MapRowRec) * B1);
        else { memcpy(hp + u_src, src->slots, 4 * B1 * M1); memcpy(hp + u_oct, last.octave, 4 * B1 * M1); memcpy(hp + u_ang, last.angle, 4 * B1 * M1); }
    }
    // map-fed rows: k_map_rows_gather behind the upload, on the same stream
    void gather(rt::stream_t s, uint8_t* dp, int B, int M) const {
        const dim3 grid((unsigned)((4 * (size_t)M + 255) / 256), B, 1), blk(256, 1, 1);
        ORBX_LAUNCH(k_map_rows_gather, grid, blk, 0, s, src->S, M, (const int*)(dp + u_n), keyframe ? (const int*)nullptr : (const int*)(dp + u_src),
                    keyframe ? (const MapRowRec*)(dp + u_src) : (const MapRowRec*)nullptr, (const uint8_t*)(dp + u_exc), dp + u_val, (float*)(dp + u_pos),
                    (unsigned long long*)(dp + u_desc), (float*)(dp + u_oct), (float*)(dp + u_mxd), (float*)(dp + u_ang));
    }
};
// The staging block goes up; rows that come from the map (U with a src; nullptr: the batch uploads no such rows) are gathered behind it.  The event of the
// staging block is recorded behind both, and a map-fed call waits for it on the host - once it has passed, the batch holds copies of everything it reads of
// the map, so the caller may release the map's mutex while the search still runs
int batch_upload(orbx_extractor* h, size_t u_total, const PointRowsUpload* U, int B, int M) {
    uint8_t* hp = h->h_lp_in.p; uint8_t* dp = h->d_lp.p;
    const bool map_fed = U && U->src;
    if (rt::copy_h2d(dp, hp, u_total, h->s0)) return fail(ORBX_E_DEVICE, "upload failed: %s", rt::last_error());
    if (map_fed) U->gather(h->s0, dp, B, M);
    if (rt::event_record(h->ev_lp, h->s0)) return fail(ORBX_E_DEVICE, "upload failed: %s", rt::last_error());
    h->lp_pending = true;
    if (map_fed && (rt::event_sync(h->ev_lp) || rt::check_launch())) return fail(ORBX_E_DEVICE, "gathering the rows from the map failed: %s", rt::last_error());
    return ORBX_OK;
}
// the fetch of the handle's pending batch: `slots` assignments per frame, `nviews` mbTrackInView arrays (fetched when fetch_views says so); as_slots: of a
// batch on a map's own sets, the assignments as map slots (the entry points have checked that it is one)
int batch_fetch(orbx_extractor* h, size_t slots, const char* what, int* assigned, int cap, int* nmatches, int nviews, bool fetch_views, uint8_t* const* views,
                bool as_slots = false) {
    rt::set_device(h->device);
    const PendingBatch& P = h->batch;
    const size_t B1 = P.B, M1 = P.M > 0 ? P.M : 0;
    const ResultBlock res(B1, slots, P.slot_result);
    // mbTrackInView on the device: frame b's M_b bytes at the prefix sum (one set for every frame: [B][M]); the caller's rows are M = max M_b apart
    size_t vb = 0;
    if (fetch_views) for (size_t b = 0; b < B1; b++) vb += (size_t)P.m(b);
    uint8_t* hp = h->h_lp_out.p;
    int e = rt::copy_d2h(hp, h->d_lp.p + P.o_result, res.bytes, h->s0);
    if (fetch_views) for (int v = 0; v < nviews; v++) e |= rt::copy_d2h(hp + al16(res.bytes) + v * vb, h->d_lp.p + P.o_view[v], vb, h->s0);
    if (e || rt::stream_sync(h->s0) || rt::check_launch()) return fail(ORBX_E_DEVICE, "%s failed: %s", what, rt::last_error());
    h->lp_pending = false;
    if (h->profile) h->stage_ms[ST_MATCH] = rt::event_elapsed_ms(h->ev_stage[ST_MATCH][0], h->ev_stage[ST_MATCH][1]);
    const int total = *(const int*)hp;
    if (P.M > 0 && (size_t)total > h->lp_pool) {                    // the candidate pool was too small: the caller enqueues again (the pool has grown)
        h->lp_pool = (size_t)total + (size_t)total / 8 + 4096;
        batch_clear(h);                                             // its entries were never written: a second fetch, now under the larger lp_pool, would pass them off as results
        return fail(ORBX_E_CAPACITY, "candidate pool overflow (%d entries): enqueue the search again, the pool has been enlarged", total);
    }
    if (nmatches) memcpy(nmatches, hp + res.nmatches, 4 * B1);
    if (assigned) {
        const int* src = (const int*)(hp + (as_slots ? res.as_slots : res.assigned));
        if ((size_t)cap == slots) memcpy(assigned, src, 4 * B1 * slots);
        else for (size_t b = 0; b < B1; b++) memcpy(assigned + b * (size_t)cap, src + b * slots, 4 * slots);
    }
    if (fetch_views) for (int v = 0; v < nviews; v++) if (views[v]) {
        const uint8_t* src = hp + al16(res.bytes) + v * vb;
        for (size_t b = 0; b < B1; b++) {
            const size_t m = (size_t)P.m(b);
            memcpy(views[v] + b * M1, src, m); memset(views[v] + b * M1 + m, 0, M1 - m);
            src += m;
        }
    }
    return ORBX_OK;
}
// the device block of a one-camera batch behind the upload (and the rows gathered from a map): uRight of "no stereo" | grid | queries | `extra` bytes of the
// caller's | q_start | q_count | result | entry pool
struct CameraBlock {
    Bump d; size_t ur; GridBlock g; size_t q, extra, qs, qc; ResultBlock r; size_t res, pool;
    CameraBlock(size_t o, size_t B1, size_t rows, size_t C1, bool no_u_right, size_t extra_bytes, bool slot_result = false)         // rows: query rows of the whole batch
        : d(o), ur(d.take(no_u_right ? 4 * B1 * C1 : 0)), g(d, B1, C1), r(B1, C1, slot_result) {
        q = d.take(sizeof(AreaQuery) * rows); extra = d.take(extra_bytes); qs = d.take(4 * rows); qc = d.take(4 * rows);
        res = d.take(r.bytes); pool = d.o;
    }
};
// frames [first, first + B) of the handle's last extraction: mvKeysUn, descriptors, counts
struct FrameRange { const KeyPointRec* kps; const unsigned long long* desc; const int* n; };
FrameRange frame_range(const orbx_extractor* h, int first) {
    const size_t o = (size_t)first * h->kp_total_cap;
    return {(h->ex_undist_active ? h->d_kps_un.p : h->d_kps.p) + o, h->d_desc.p + o * 4, h->d_nm.p + first};
}
// the grid of the frames, then the window searches of the query set into the entry pool.  queries(): the launch that writes the queries (and zeroes the pool
// counter).  maps (device): the table of the frames' query rows and descriptors, M the largest of its M_b.  gate_right: the window search applies the
// right-coordinate gate, against mvuRight of the extraction or, without use_u_right, against "no stereo"
template <typename Queries>
void camera_searches(orbx_extractor* h, const FrameRange& F, int B, int M, const CameraBlock& K, uint8_t* dp, const GridParams& g, const FrameMapRec* maps, size_t pool,
                     int use_u_right, int gate_right, const Queries& queries) {
    const int cap = h->kp_total_cap;
    const float* ur = h->d_uRight.p;
    if (!use_u_right) { rt::memset_async(dp + K.ur, 0xBF, 4 * (size_t)B * cap, h->s0); ur = (const float*)(dp + K.ur); }   // 0xBFBFBFBF = -1.498...: a negative uRight = monocular keypoint
    int* d_counter = (int*)(dp + K.res);
    if (h->profile) rt::event_record(h->ev_stage[ST_MATCH][0], h->s0);
    {
        dim3 grid(B, 1, 1), blkg(kGridThreads, 1, 1);
        ORBX_LAUNCH(k_grid_build, grid, blkg, 0, h->s0, F.kps, 0, g, (int*)(dp + K.g.cof), (int*)(dp + K.g.cst), (int*)(dp + K.g.cit), F.n, cap);
    }
    if (M <= 0) { rt::memset_async(d_counter, 0, 16, h->s0); return; }
    queries();
    const dim3 grid((M + 255) / 256, B, 1), blk(256, 1, 1);              // M: of the one set, or the largest of the frames' own
    ORBX_LAUNCH(k_area_search_threads, grid, blk, 0, h->s0, (const AreaQuery*)(dp + K.q), maps, F.kps, ur, F.desc, g, (const int*)(dp + K.g.cst), (const int*)(dp + K.g.cit),
                gate_right, d_counter, (int)pool, (int*)(dp + K.qs), (int*)(dp + K.qc), (int2*)(dp + K.pool), cap);
}
// orbm_search_local_points_batch (one resident set, `maps` == NULL) and orbm_search_local_points_batch_maps (maps[b] = frame b's own)
int local_points_batch(orbx_extractor* h, int first, int B, const OrbmFrustumView* frames, const orbm_points* points, const uint8_t* is_bad, const uint8_t* has_obs,
                       const OrbmFrameMap* maps, const uint8_t* occupied, int use_u_right, float cos_limit, float th, int far_points, float th_far, float nnratio,
                       int want_in_view, const MapSetRec* sets = nullptr) {
    if (!h || !frames || (!points && !maps && !sets) || B <= 0 || first < 0 || first + B > h->lastB) return fail(ORBX_E_ARG, "bad frame range / null");
    BatchMaps P{points, is_bad, has_obs, maps, B, sets};
    if (int rc = P.plan(h->device)) return rc;
    if (int rc = frames_check(frames, sizeof *frames, B)) return rc;
    if (undistort_stale(h)) return fail(ORBX_E_ARG, "orbx_set_undistort was called after the last extraction: extract again before searching its frames");
    rt::set_device(h->device);
    const int M = P.m_max, cap = h->kp_total_cap;
    const size_t B1 = B, C1 = cap, rows = P.rows;
    const size_t smem_accept = 4 * (size_t)((cap + 31) / 32) + 4 * (size_t)cap + 64;
    if (smem_accept + 1024 > rt::lds_limit(h->device)) return fail(ORBX_E_CAPACITY, "%d keypoints per frame need %zu bytes of LDS in the accept kernel", cap, smem_accept);
    // upload block: poses | the table of per-frame maps | bad flags | has-observation flags | occupancy.  On a map's own sets the flags are not uploaded:
    // the table of k_map_set_flags goes up in their place and the flag blocks lie behind the upload, where that kernel writes them
    Bump u;
    const size_t u_f = u.take(sizeof(FrustumParams) * B1), u_tab = u.take(P.table_bytes()), up_bad = u.take(sets ? 0 : P.flags), up_obs = u.take(sets ? 0 : P.flags),
                 u_occ = u.take(occupied ? B1 * C1 : 0), u_ftab = u.take(P.flag_table_bytes()), u_total = u.o;
    Bump behind(u_total);
    const size_t u_bad = sets ? behind.take(P.flags) : up_bad, u_obs = sets ? behind.take(P.flags) : up_obs;
    // between the queries and their CSR: track [5 rows] | level [rows] | in_view [rows]   (rows: the sum of the frames' M_b; B x M for one set)
    Bump t;
    const size_t o_trk = t.take(20 * rows), o_lvl = t.take(4 * rows), o_view = t.take(rows);
    const CameraBlock K(behind.o, B1, rows, C1, !use_u_right, t.o, sets != nullptr);
    const size_t pool = batch_pool(h, rows * 6 + 4096);
    if (!batch_reserve(h, K.pool, pool, u_total, al16(K.r.bytes) + (want_in_view ? rows : 0)))
        return fail(ORBX_E_DEVICE, "allocation failed (batched local point search, %d frames, %zu points)", B, rows);
    uint8_t* hp = h->h_lp_in.p; uint8_t* dp = h->d_lp.p; uint8_t* dx = dp + K.extra;
    FrustumParams* Fp = (FrustumParams*)(hp + u_f);
    for (int b = 0; b < B; b++) fill_frustum_params(&frames[b], cos_limit, th, far_points, th_far, &Fp[b]);
    P.stage(hp + u_tab, hp + up_bad, hp + up_obs);
    if (sets) P.flag_table(hp + u_ftab);
    if (occupied) memcpy(hp + u_occ, occupied, B1 * C1);
    if (int rc = batch_upload(h, u_total, nullptr, B, M)) return rc;
    if (sets) P.gather_flags(h->s0, dp + u_ftab, dp + u_bad, dp + u_obs);
    const FrameRange F = frame_range(h, first);
    const FrameMapRec* d_tab = (const FrameMapRec*)(dp + u_tab);
    camera_searches(h, F, B, M, K, dp, grid_from_view(frames[0]), d_tab, pool, use_u_right, 1, [&]() {
        const dim3 grid((M + 255) / 256, B, 1), blk(256, 1, 1);
        ORBX_LAUNCH(k_frustum_batch, grid, blk, 0, h->s0, (const FrustumParams*)(dp + u_f), d_tab, (const uint8_t*)(dp + u_bad), dx + o_view, (float*)(dx + o_trk),
                    (int*)(dx + o_lvl), (AreaQuery*)(dp + K.q), (int*)(dp + K.res));
    });
    {
        dim3 grida(B, 1, 1), blka(64, 1, 1);
        const uint8_t* d_occ = occupied ? (const uint8_t*)(dp + u_occ) : (const uint8_t*)nullptr;
        ORBX_LAUNCH(k_local_accept, grida, blka, smem_accept, h->s0, d_tab, cap, F.n, (const int*)(dp + K.qs), (const int*)(dp + K.qc), (const int2*)(dp + K.pool), d_occ,
                    (const uint8_t*)(dp + u_obs), nnratio, TH_HIGH, (int*)(dp + K.res + K.r.assigned), (int*)(dp + K.res + K.r.nmatches));
    }
    if (sets) P.translate(h->s0, dp + u_ftab, (const int*)(dp + K.res + K.r.assigned), cap, (int*)(dp + K.res + K.r.as_slots));
    return batch_finish(h, {B, M, P.M, K.res, {K.extra + o_view, 0}, want_in_view != 0, false, sets != nullptr});
}
}  // namespace
extern "C" {

int orbm_search_local_points_batch(orbx_extractor* h, int first, int B, const OrbmFrustumView* frames, const orbm_points* points, const uint8_t* is_bad,
                                   const uint8_t* has_obs, const uint8_t* occupied, int use_u_right, float cos_limit, float th, int far_points, float th_far,
                                   float nnratio, int want_in_view) {
    batch_clear(h);
    return local_points_batch(h, first, B, frames, points, is_bad, has_obs, nullptr, occupied, use_u_right, cos_limit, th, far_points, th_far, nnratio, want_in_view);
}

int orbm_search_local_points_batch_maps(orbx_extractor* h, int first, int B, const OrbmFrustumView* frames, const OrbmFrameMap* maps, const uint8_t* occupied,
                                        int use_u_right, float cos_limit, float th, int far_points, float th_far, float nnratio, int want_in_view) {
    batch_clear(h);
    if (h && !maps) return fail(ORBX_E_ARG, "null table of per-frame maps");
    return local_points_batch(h, first, B, frames, nullptr, nullptr, nullptr, maps, occupied, use_u_right, cos_limit, th, far_points, th_far, nnratio, want_in_view);
}

int orbm_points_count(const orbm_points* p) { return p ? p->M : 0; }

namespace {
// SearchByProjection(CurrentFrame, LastFrame) (keyframe = false) or (CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (keyframe = true) for B frames.
// src == nullptr: the rows are the caller's arrays; else they are read from the map (the caller holds its mutex until this returns).  The entry points have
// checked their own arguments (h among them) and cleared the pending batch
int projection_batch(orbx_extractor* h, int first, int B, const OrbmFrustumView* cur, const PointRows* last, float th, const uint8_t* forward, const uint8_t* backward,
                     int check_ori, const uint8_t* occupied, int use_u_right, bool keyframe, int th_accept, const MapRows* src = nullptr) {
    const int M = last->cap;
    if (int rc = frames_check(cur, sizeof *cur, B)) return rc;
    for (int b = 0; b < B; b++) if (last->n[b] < 0 || last->n[b] > M) return fail(ORBX_E_ARG, "frame %d: %d points in %d rows", b, last->n[b], M);
    if (undistort_stale(h)) return fail(ORBX_E_ARG, "orbx_set_undistort was called after the last extraction: extract again before searching its frames");
    rt::set_device(h->device);
    const int cap = h->kp_total_cap;
    const size_t B1 = B, M1 = M, C1 = cap;
    const size_t smem_accept = 4 * (size_t)((cap + 31) / 32) + 4 * (size_t)cap + 4 * (size_t)M + 64;          // grows with cap_last: checked before anything is enqueued
    if (smem_accept + 1024 > rt::lds_limit(h->device)) return fail(ORBX_E_CAPACITY, "%d keypoints and %d last-frame points per frame need %zu bytes of LDS in the accept kernel", cap, M, smem_accept);
    // upload block: poses | the table of the frames' rows | the rows (n_last .. descriptors) | occupancy | a key frame's mfMaxDistance rows
    Bump u;
    const size_t u_f = u.take(sizeof(FrustumParams) * B1), u_tab = u.take(sizeof(FrameMapRec) * B1);
    PointRowsUpload U(u, B1, M1, src, keyframe);
    const size_t u_occ = u.take(occupied ? B1 * C1 : 0), u_mxd_up = u.take(keyframe && !src ? 4 * B1 * M1 : 0), u_total = u.o;
    Bump behind(u_total);
    U.device_rows(behind, B1, M1);                              // (map-fed: the gathered rows between the upload and the camera block)
    const size_t u_mxd = src ? U.u_mxd : u_mxd_up;
    const CameraBlock K(behind.o, B1, B1 * M1, C1, !use_u_right, 0);
    const size_t pool = batch_pool(h, B1 * M1 * 16 + 4096);                     // th = 7 .. 15 px windows: a dozen candidates per point
    if (!batch_reserve(h, K.pool, pool, u_total, al16(K.r.bytes)))
        return fail(ORBX_E_DEVICE, "allocation failed (batched last-frame search, %d frames x %d points)", B, M);
    uint8_t* hp = h->h_lp_in.p; uint8_t* dp = h->d_lp.p;
    FrustumParams* Fp = (FrustumParams*)(hp + u_f);
    for (int b = 0; b < B; b++) {
        fill_frustum_params(&cur[b], 0.0f, th, 0, 0.0f, &Fp[b]);
        Fp[b].forward = forward ? forward[b] != 0 : 0; Fp[b].backward = backward ? backward[b] != 0 : 0; Fp[b].debug_flags = h->debug_stereo_flags;
    }
    U.stage(hp, *last, B1, M1);
    stage_uniform_table(hp + u_tab, B, M, (const unsigned long long*)(dp + U.u_desc));
    if (keyframe && !src) memcpy(hp + u_mxd, last->max_distance, 4 * B1 * M1);
    if (occupied) memcpy(hp + u_occ, occupied, B1 * C1);
    if (int rc = batch_upload(h, u_total, &U, B, M)) return rc;
    const FrameRange F = frame_range(h, first);
    const FrameMapRec* d_tab = (const FrameMapRec*)(dp + u_tab);
    camera_searches(h, F, B, M, K, dp, grid_from_view(cur[0]), d_tab, pool, use_u_right, keyframe ? 0 : 1, [&]() {
        const dim3 grid((M + 255) / 256, B, 1), blk(256, 1, 1);
        if (keyframe) ORBX_LAUNCH(k_keyframe_queries, grid, blk, 0, h->s0, (const FrustumParams*)(dp + u_f), M, (const int*)(dp + U.u_n), (const float*)(dp + U.u_pos),
                                  (const uint8_t*)(dp + U.u_val), (const float*)(dp + U.u_oct), (const float*)(dp + u_mxd), (AreaQuery*)(dp + K.q), (int*)(dp + K.res));
        else ORBX_LAUNCH(k_lastframe_queries, grid, blk, 0, h->s0, (const FrustumParams*)(dp + u_f), M, (const int*)(dp + U.u_n), (const float*)(dp + U.u_pos),
                         (const uint8_t*)(dp + U.u_val), (const int*)(dp + U.u_oct), (AreaQuery*)(dp + K.q), (int*)(dp + K.res));
    });
    {
        dim3 grid(B, 1, 1), blka(64, 1, 1);
        ORBX_LAUNCH(k_lastframe_accept, grid, blka, smem_accept, h->s0, d_tab, cap, F.n, (const int*)(dp + K.qs), (const int*)(dp + K.qc), (const int2*)(dp + K.pool),
                    occupied ? (const uint8_t*)(dp + u_occ) : (const uint8_t*)nullptr, (const uint8_t*)(dp + U.u_obs), th_accept, (int*)(dp + K.res + K.r.assigned),
                    (int*)(dp + K.res + K.r.nmatches), (const float*)(dp + U.u_ang), F.kps, check_ori);
    }
    return batch_finish(h, {B, M, {}, K.res, {0, 0}, false, false});
}
}  // namespace

int orbm_search_by_projection_lastframe_batch(orbx_extractor* h, int first, int B, const OrbmFrustumView* cur, const OrbmLastFrameBatch* last, float th,
                                              const uint8_t* forward, const uint8_t* backward, int check_ori, const uint8_t* occupied, int use_u_right) {
    batch_clear(h);
    if (!h || !cur || !last || B <= 0 || first < 0 || first + B > h->lastB) return fail(ORBX_E_ARG, "bad frame range / null");
    if (last->cap_last <= 0 || !last->n || !last->pos || !last->valid || !last->octave || !last->angle || !last->desc) return fail(ORBX_E_ARG, "bad last-frame batch");
    const PointRows R = last_frame_rows(last);
    return projection_batch(h, first, B, cur, &R, th, forward, backward, check_ori, occupied, use_u_right, false, TH_HIGH);
}

int orbm_search_by_projection_keyframe_batch(orbx_extractor* h, int first, int B, const OrbmFrustumView* cur, const OrbmKeyFramePointBatch* kf, float th, int orb_dist,
                                             int check_ori, const uint8_t* occupied) {
    batch_clear(h);
    if (!h || !cur || !kf || B <= 0 || first < 0 || first + B > h->lastB) return fail(ORBX_E_ARG, "bad frame range / null");
    if (kf->cap_kf <= 0 || !kf->n || !kf->pos || !kf->valid || !kf->min_distance || !kf->max_distance || !kf->angle || !kf->desc) return fail(ORBX_E_ARG, "bad key-frame batch");
    if (orb_dist < 0 || orb_dist > 256) return fail(ORBX_E_ARG, "ORBdist out of range");
    // every accepted point occupies its keypoint (`if(CurrentFrame.mvpMapPoints[i2]) continue;`, :2259-2260): has_obs = all, and no right-coordinate gate
    const PointRows R = {kf->cap_kf, kf->n, kf->pos, kf->valid, nullptr, kf->angle, nullptr, kf->desc, kf->min_distance, kf->max_distance};
    return projection_batch(h, first, B, cur, &R, th, nullptr, nullptr, check_ori, occupied, /*use_u_right*/ 0, true, orb_dist);
}

int orbm_search_local_points_fetch(orbx_extractor* h, int* assigned, int cap, int* nmatches, uint8_t* in_view) {
    if (!h || h->batch.B <= 0) return fail(ORBX_E_ARG, "no batched local point search is pending");
    if (h->batch.rig) return fail(ORBX_E_ARG, "the pending batch is a rig batch: fetch it with orbm_search_rig_batch_fetch");
    if (assigned && cap < h->kp_total_cap) return fail(ORBX_E_CAPACITY, "assigned rows need %d entries", h->kp_total_cap);
    const bool fetch_view = in_view && h->batch.want_view && h->batch.M > 0;
    const int rc = batch_fetch(h, h->kp_total_cap, "batched local point search", assigned, cap, nmatches, 1, fetch_view, &in_view);
    if (rc) return rc;
    if (in_view && !fetch_view) return fail(ORBX_E_ARG, "in_view was not requested at enqueue time");
    return ORBX_OK;
}

int orbm_search_by_projection_frame(orbx_extractor* h, const OrbmFrameView* Cur, const OrbmLastFrameView* Last, float th, int forward, int backward,
                                    int check_ori, int* assigned, int* nmatches_out) {
    if (!h || !Cur || !Last || !assigned) return fail(ORBX_E_ARG, "null");
    rt::set_device(h->device);
    DeviceFrame D;
    int rc = upload_frame(h, Cur, &D); if (rc) return rc;
    const int NL = Last->N, N = Cur->N;
    std::vector<AreaQuery> qs(NL);
    for (int i = 0; i < NL; i++) {
        AreaQuery& q = qs[i]; memset(&q, 0, sizeof q);
        if (!Last->valid[i]) continue;
        const float u = Last->proj_u[i], v = Last->proj_v[i];
        if (u < Cur->min_x || u > Cur->max_x) continue;                  // :2003-2006
        if (v < Cur->min_y || v > Cur->max_y) continue;
        const int oct = Last->octave[i];
        if (oct < 0 || oct >= Cur->nlevels) continue;
        q.x = u; q.y = v; q.r = th * Cur->scale_factors[oct];            // :2012
        q.ur = u - Cur->mbf * Last->inv_z[i];                            // :2045
        if (forward) { q.min_level = oct; q.max_level = -1; }            // :2018-2023
        else if (backward) { q.min_level = 0; q.max_level = oct; }
        else { q.min_level = oct - 1; q.max_level = oct + 1; }
        q.active = 1; q.gate = 1;
    }
    Cands c;
    rc = run_area_search(h, D, qs, Last->desc, &c); if (rc) return rc;
    std::vector<uint8_t> occ(N > 0 ? N : 1, 0);
    if (Cur->occupied) memcpy(occ.data(), Cur->occupied, N);
    for (int i = 0; i < N; i++) assigned[i] = -1;
    RotHist hist;
    int nmatches = 0;
    for (int i = 0; i < NL; i++) {
        if (!qs[i].active || c.count[i] == 0) continue;
        const Best b = scan_best(c, i, occ.data());
        if (b.dist <= TH_HIGH) {
            assigned[b.idx] = i;
            occ[b.idx] = Last->has_obs ? Last->has_obs[i] : 1;
            nmatches++;
            if (check_ori) hist.add(Last->angle[i], Cur->keys_un[b.idx].angle, b.idx);
        }
    }
    if (check_ori) hist.prune([&](int idx) { assigned[idx] = -2; nmatches--; });
    if (nmatches_out) *nmatches_out = nmatches;
    return ORBX_OK;
}

// ORBmatcher::SearchForTriangulation for one key frame against n2 neighbours in a single launch (LocalMapping::CreateNewMapPoints calls
// it for 10-30 neighbours in a row, src/LocalMapping.cc:510-540).  matches12: n2 rows of K1->N entries.
static int search_for_triangulation_impl(orbx_extractor* h, const OrbmKeyFrameView* K1, int n2, const OrbmKeyFrameView* const* K2s, const float* F12s,
                                         const float* eps, const OrbmKB8Pair* kb8, int only_stereo, int coarse, int check_ori, int* matches12, int* nmatches_out) {
    if (!h || !K1 || n2 < 0 || (n2 > 0 && (!K2s || (!F12s && !kb8) || !eps || !matches12))) return fail(ORBX_E_ARG, "null");
    if (K1->N >= 65535) return fail(ORBX_E_ARG, "keyframe too large");
    rt::set_device(h->device);
    const int N1 = K1->N;
    for (size_t i = 0; i < (size_t)n2 * N1; i++) matches12[i] = -1;
    for (int j = 0; j < n2; j++) if (nmatches_out) nmatches_out[j] = 0;
    // merge-join of the feature vectors by node id (:1105-1286); one work item per unmatched feature of KF1 and neighbour.
    // The neighbours' arrays are concatenated; feat2 entries and the returned indices are global (base2[j] + index in KF j).
    std::vector<BowItem> items;
    std::vector<int> base2(n2 + 1, 0), fbase(n2 + 1, 0), first_item(n2 + 1, 0);
    for (int j = 0; j < n2; j++) {
        const OrbmKeyFrameView* K2 = K2s[j];
        if (!K2 || K2->N >= 65535 || K2->nlevels > kMaxLevels) return fail(ORBX_E_ARG, "bad neighbour key frame %d", j);
        base2[j + 1] = base2[j] + K2->N; fbase[j + 1] = fbase[j] + K2->fv_start[K2->fv_nodes];
        first_item[j] = (int)items.size();
        bool node_too_large = false;
        for_each_common_node(K1, K2, [&](int a, int b) {
            for (int k = K1->fv_start[a]; k < K1->fv_start[a + 1]; k++) {
                const int idx1 = (int)K1->fv_feat[k];
                if (K1->has_map_point && K1->has_map_point[idx1]) continue;
                const bool stereo1 = K1->u_right && K1->u_right[idx1] >= 0;
                if (only_stereo && !stereo1) continue;
                BowItem it; it.idx1 = idx1; it.start2 = fbase[j] + K2->fv_start[b]; it.cnt2 = K2->fv_start[b + 1] - K2->fv_start[b]; it.out_off = j;
                node_too_large |= it.cnt2 > 0xFFFF;
                items.push_back(it);
            }
        });
        if (node_too_large) return fail(ORBX_E_ARG, "vocabulary node with more than 65535 features");
    }
    first_item[n2] = (int)items.size();
    if (items.empty()) return ORBX_OK;
    const int T2 = std::max(base2[n2], 1), TF = std::max(fbase[n2], 1);
    std::vector<float> ur1(N1 > 0 ? N1 : 1, -1.0f), ur2(T2, -1.0f);
    if (K1->u_right) memcpy(ur1.data(), K1->u_right, sizeof(float) * N1);
    std::vector<uint8_t> mp2(T2, 0), desc2((size_t)T2 * 32);
    std::vector<KeyPointRec> kps2(T2);
    std::vector<int> feat2(TF);
    std::vector<BowParams> Ps(n2);
    for (int j = 0; j < n2; j++) {
        const OrbmKeyFrameView* K2 = K2s[j];
        const int N2 = K2->N, o = base2[j];
        if (N2 > 0) { memcpy(&kps2[o], K2->keys_un, sizeof(KeyPointRec) * (size_t)N2); memcpy(&desc2[(size_t)o * 32], K2->desc, 32 * (size_t)N2); }
        if (K2->u_right) memcpy(&ur2[o], K2->u_right, sizeof(float) * (size_t)N2);
        if (K2->has_map_point) memcpy(&mp2[o], K2->has_map_point, N2);
        const int nf = K2->fv_start[K2->fv_nodes];
        for (int k = 0; k < nf; k++) feat2[fbase[j] + k] = (int)K2->fv_feat[k] + o;
        BowParams& P = Ps[j]; memset(&P, 0, sizeof P);
        if (F12s) for (int i = 0; i < 9; i++) P.F12[i] = F12s[9 * (size_t)j + i];
        if (kb8) fill_kb8(P, kb8[j], K1->level_sigma2, K1->nlevels);         // Kannala-Brandt cameras: one OrbmKB8Pair per neighbour
        P.ep[0] = eps[2 * (size_t)j]; P.ep[1] = eps[2 * (size_t)j + 1];
        for (int l = 0; l < K2->nlevels; l++) { P.scale2[l] = K2->scale_factors[l]; P.sigma2_2[l] = K2->level_sigma2[l]; }
        P.only_stereo = only_stereo; P.coarse = coarse; P.th_low = TH_LOW;
    }
    Packer pk(h);
    const size_t pk1 = pk.add(K1->keys_un, sizeof(KeyPointRec) * (size_t)N1), pd1 = pk.add(K1->desc, 32 * (size_t)N1), pu1 = pk.add(ur1.data(), sizeof(float) * ur1.size()),
                 pk2 = pk.add(kps2.data(), sizeof(KeyPointRec) * kps2.size()), pd2 = pk.add(desc2.data(), desc2.size()), pu2 = pk.add(ur2.data(), sizeof(float) * ur2.size()),
                 pm2 = pk.add(mp2.data(), mp2.size()), pit = pk.add(items.data(), sizeof(BowItem) * items.size()), pf2 = pk.add(feat2.data(), sizeof(int) * feat2.size()),
                 pps = pk.add(Ps.data(), sizeof(BowParams) * Ps.size());
    if (pk.flush() || h->d_si[SI_BEST].ensure(items.size())) return fail(ORBX_E_DEVICE, "upload/allocation failed");
    dim3 grid(((int)items.size() + 3) / 4, 1, 1), blk(256, 1, 1);
    if (kb8)
        ORBX_LAUNCH(k_bow_search_kb8, grid, blk, 0, h->s0, pk.dev<BowItem>(pit), (int)items.size(),
                    pk.dev<KeyPointRec>(pk1), pk.dev<unsigned long long>(pd1), pk.dev<float>(pu1),
                    pk.dev<KeyPointRec>(pk2), pk.dev<unsigned long long>(pd2), pk.dev<float>(pu2),
                    pk.dev<uint8_t>(pm2), pk.dev<int>(pf2), pk.dev<BowParams>(pps), h->d_si[SI_BEST].p);
    else
    ORBX_LAUNCH(k_bow_search, grid, blk, 0, h->s0, pk.dev<BowItem>(pit), (int)items.size(),
                pk.dev<KeyPointRec>(pk1), pk.dev<unsigned long long>(pd1), pk.dev<float>(pu1),
                pk.dev<KeyPointRec>(pk2), pk.dev<unsigned long long>(pd2), pk.dev<float>(pu2),
                pk.dev<uint8_t>(pm2), pk.dev<int>(pf2), pk.dev<BowParams>(pps), h->d_si[SI_BEST].p);
    std::vector<int> best(items.size());
    if (fetch_sync(h, best.data(), h->d_si[SI_BEST].p, sizeof(int) * items.size()) || rt::check_launch())
        return fail(ORBX_E_DEVICE, "bow search failed: %s", rt::last_error());
    for (int j = 0; j < n2; j++) {
        const OrbmKeyFrameView* K2 = K2s[j];
        int* m12 = matches12 + (size_t)j * N1;
        int nmatches = 0;
        RotHist hist;
        for (int k = first_item[j]; k < first_item[j + 1]; k++) {
            if (best[k] < 0) continue;
            const int idx1 = items[k].idx1, idx2 = best[k] - base2[j];
            m12[idx1] = idx2;
            nmatches++;
            if (check_ori) hist.add(K1->keys_un[idx1].angle, K2->keys_un[idx2].angle, idx1);
        }
        if (check_ori) hist.prune([&](int idx1) { m12[idx1] = -1; nmatches--; });           // :1270-1286
        if (nmatches_out) nmatches_out[j] = nmatches;
    }
    return ORBX_OK;
}

int orbm_search_for_triangulation_batch(orbx_extractor* h, const OrbmKeyFrameView* K1, int n2, const OrbmKeyFrameView* const* K2s, const float* F12s,
                                        const float* eps, int only_stereo, int coarse, int check_ori, int* matches12, int* nmatches_out) {
    if (n2 > 0 && !F12s) return fail(ORBX_E_ARG, "null");
    return search_for_triangulation_impl(h, K1, n2, K2s, F12s, eps, nullptr, only_stereo, coarse, check_ori, matches12, nmatches_out);
}

int orbm_search_for_triangulation_kb8(orbx_extractor* h, const OrbmKeyFrameView* K1, const OrbmKeyFrameView* K2, const OrbmKB8Pair* cams, const float ep[2],
                                      int only_stereo, int coarse, int check_ori, int* matches12, int* nmatches_out) {
    if (!h || !K1 || !K2 || !cams || !ep || !matches12) return fail(ORBX_E_ARG, "null");
    return search_for_triangulation_impl(h, K1, 1, &K2, nullptr, ep, cams, only_stereo, coarse, check_ori, matches12, nmatches_out);
}

int orbm_search_for_triangulation(orbx_extractor* h, const OrbmKeyFrameView* K1, const OrbmKeyFrameView* K2, const float F12[9], const float ep[2],
                                  int only_stereo, int coarse, int check_ori, int* matches12, int* nmatches_out) {
    if (!h || !K1 || !K2 || !F12 || !ep || !matches12) return fail(ORBX_E_ARG, "null");
    return orbm_search_for_triangulation_batch(h, K1, 1, &K2, F12, ep, only_stereo, coarse, check_ori, matches12, nmatches_out);
}


// ORBmatcher::SearchByBoW, both overloads (src/ORBmatcher.cc:259-493, :892-1043), non-fisheye path, for n independent (K1, K2) pairs in one
// launch: Tracking::Relocalization matches every candidate key frame against the current frame (src/Tracking.cc:4360-4380), loop / merge
// detection one key frame against its candidates' covisible key frames (src/LoopClosing.cc:840-850).  The pairs' descriptors and feature
// lists are concatenated (indices made global), one k_bow_dists launch computes every node-bucket distance, the order-dependent selection
// is replayed per pair on the host.
int orbm_search_by_bow_batch(orbx_extractor* h, int n, const OrbmKeyFrameView* const* K1s, const OrbmKeyFrameView* const* K2s, float nnratio, int th_inclusive,
                             int check_ori, int* const* matches12, int* nmatches_out) {
    if (!h || n < 0 || (n > 0 && (!K1s || !K2s || !matches12))) return fail(ORBX_E_ARG, "null");
    rt::set_device(h->device);
    std::vector<BowItem> items;
    std::vector<int> first_item(n + 1, 0), base1(n + 1, 0), base2(n + 1, 0), fbase2(n + 1, 0), obase(n + 1, 0);
    int total = 0;
    for (int p = 0; p < n; p++) {
        const OrbmKeyFrameView *K1 = K1s[p], *K2 = K2s[p];
        if (!K1 || !K2 || !matches12[p] || K1->N >= 65535 || K2->N >= 65535) return fail(ORBX_E_ARG, "bad key frame pair %d", p);
        for (int i = 0; i < K1->N; i++) matches12[p][i] = -1;
        if (nmatches_out) nmatches_out[p] = 0;
        first_item[p] = (int)items.size(); obase[p] = total;
        base1[p + 1] = base1[p] + K1->N; base2[p + 1] = base2[p] + K2->N; fbase2[p + 1] = fbase2[p] + K2->fv_start[K2->fv_nodes];
        for_each_common_node(K1, K2, [&](int a, int b) {
            for (int k = K1->fv_start[a]; k < K1->fv_start[a + 1]; k++) {
                const int idx1 = (int)K1->fv_feat[k];
                if (!K1->has_map_point || !K1->has_map_point[idx1]) continue;     // !pMP || pMP->isBad()
                BowItem it; it.idx1 = base1[p] + idx1; it.start2 = fbase2[p] + K2->fv_start[b]; it.cnt2 = K2->fv_start[b + 1] - K2->fv_start[b]; it.out_off = total;
                total += it.cnt2;
                items.push_back(it);
            }
        });
    }
    first_item[n] = (int)items.size(); obase[n] = total;
    if (items.empty() || total == 0) return ORBX_OK;
    const int T1 = std::max(base1[n], 1), T2 = std::max(base2[n], 1), TF = std::max(fbase2[n], 1);
    std::vector<uint8_t> desc1((size_t)T1 * 32), desc2((size_t)T2 * 32), elig(T2, 1);
    std::vector<int> feat2(TF);
    for (int p = 0; p < n; p++) {
        const OrbmKeyFrameView *K1 = K1s[p], *K2 = K2s[p];
        if (K1->N > 0) memcpy(&desc1[(size_t)base1[p] * 32], K1->desc, 32 * (size_t)K1->N);
        if (K2->N > 0) memcpy(&desc2[(size_t)base2[p] * 32], K2->desc, 32 * (size_t)K2->N);
        if (K2->has_map_point) memcpy(&elig[base2[p]], K2->has_map_point, K2->N);
        const int nf = K2->fv_start[K2->fv_nodes];
        for (int k = 0; k < nf; k++) feat2[fbase2[p] + k] = (int)K2->fv_feat[k] + base2[p];
    }
    Packer pk(h);
    const size_t pd1 = pk.add(desc1.data(), desc1.size()), pd2 = pk.add(desc2.data(), desc2.size()), pel = pk.add(elig.data(), elig.size()),
                 pit = pk.add(items.data(), sizeof(BowItem) * items.size()), pf2 = pk.add(feat2.data(), sizeof(int) * feat2.size());
    if (pk.flush() || h->d_si[SI_BEST].ensure((size_t)total + 1)) return fail(ORBX_E_DEVICE, "upload/allocation failed");
    dim3 grid(((int)items.size() + 3) / 4, 1, 1), blk(256, 1, 1);
    ORBX_LAUNCH(k_bow_dists, grid, blk, 0, h->s0, pk.dev<BowItem>(pit), (int)items.size(), pk.dev<unsigned long long>(pd1), pk.dev<unsigned long long>(pd2),
                pk.dev<uint8_t>(pel), pk.dev<int>(pf2), h->d_si[SI_BEST].p);
    std::vector<int> dist((size_t)total);
    if (fetch_sync(h, dist.data(), h->d_si[SI_BEST].p, sizeof(int) * (size_t)total) || rt::check_launch())
        return fail(ORBX_E_DEVICE, "bow distances failed: %s", rt::last_error());
    for (int p = 0; p < n; p++) {
        const OrbmKeyFrameView *K1 = K1s[p], *K2 = K2s[p];
        const int N2 = K2->N;
        int* m12 = matches12[p];
        int nmatches = 0;
        // sequential replay: a target taken by an earlier feature is skipped (:331 vpMapPointMatches[realIdxF], :948 vbMatched2[idx2])
        std::vector<uint8_t> taken(N2 > 0 ? N2 : 1, 0);
        RotHist hist;
        for (int q = first_item[p]; q < first_item[p + 1]; q++) {
            const BowItem& it = items[q];
            const int idx1 = it.idx1 - base1[p];
            int bestDist1 = 256, bestIdx2 = -1, bestDist2 = 256;
            for (int j = 0; j < it.cnt2; j++) {
                const int idx2 = feat2[it.start2 + j] - base2[p];
                const int d = dist[(size_t)it.out_off + j];
                if (taken[idx2] || d < 0) continue;
                if (d < bestDist1) { bestDist2 = bestDist1; bestDist1 = d; bestIdx2 = idx2; }
                else if (d < bestDist2) bestDist2 = d;
            }
            const bool pass = th_inclusive ? (bestDist1 <= TH_LOW) : (bestDist1 < TH_LOW);
            if (pass && static_cast<float>(bestDist1) < nnratio * static_cast<float>(bestDist2)) {
                m12[idx1] = bestIdx2;
                taken[bestIdx2] = 1;
                nmatches++;
                if (check_ori) hist.add(K1->keys_un[idx1].angle, K2->keys_un[bestIdx2].angle, idx1);
            }
        }
        if (check_ori) hist.prune([&](int idx1) { m12[idx1] = -1; nmatches--; });
        if (nmatches_out) nmatches_out[p] = nmatches;
    }
    return ORBX_OK;
}

// ---- device-resident key frames ------------------------------------------------------------------------------------------------
// What the vocabulary-bucket searches read of a key frame (keys, descriptors, mvuRight, mFeatVec) is uploaded once; the searches then move
// only their call-time state (map point flags, poses) to the device and their result back.  The host keeps the angles for the
// rotation-consistency histograms and the per-level scales.
// The bucket grid of a resident key frame (Frame::AssignFeaturesToGrid) for one set of image bounds, built on the first orbm_fuse_candidates_batch that asks for
// it and kept with the key frame: mem = cell_start [kGridCellStride] | cell_items [N + 1] | cell_of [N + 1].  users: calls in flight that read it (a grid in use
// is never dropped); built: the kernel that fills it has run (an entry whose call failed before that is dropped by the next lookup).  Key frames are shared
// between the handles - and threads - of a device, so the lists are only touched under kf_grid_mutex().
struct KfGrid { float key[4]; int* mem; int users; bool built; };
struct orbm_keyframe {
    int device = 0, N = 0, fv_nodes = 0, nlevels = 0;
    uint8_t* dmem = nullptr;
    ResidentKF dev;
    std::vector<float> angle;
    float scale[kMaxLevels], sigma2[kMaxLevels];
    std::vector<KfGrid*> grids;
};
static std::mutex& kf_grid_mutex() { static std::mutex m; return m; }

int orbm_keyframe_create(orbx_extractor* h, const OrbmKeyFrameView* K, orbm_keyframe** out) {
    if (!h || !K || !out || K->N < 0 || K->fv_nodes < 0 || (K->N > 0 && (!K->keys_un || !K->desc))) return fail(ORBX_E_ARG, "bad key frame view");
    if (K->N >= 65535 || K->nlevels > kMaxLevels) return fail(ORBX_E_ARG, "key frame too large");
    if (K->fv_nodes > 0 && (!K->fv_node_id || !K->fv_start || !K->fv_feat)) return fail(ORBX_E_ARG, "bad feature vector");
    rt::set_device(h->device);
    const int N = K->N, N1 = std::max(N, 1), nn = K->fv_nodes, nf = nn > 0 ? K->fv_start[nn] : 0;
    const size_t okp = 0, odesc = okp + al16(sizeof(KeyPointRec) * (size_t)N1), our = odesc + al16(32 * (size_t)N1), onid = our + al16(4 * (size_t)N1),
                 ost = onid + al16(4 * (size_t)(nn + 1)), oft = ost + al16(4 * (size_t)(nn + 1)), onof = oft + al16(4 * (size_t)(nf + 1)),
                 total = onof + al16(4 * (size_t)N1);
    std::vector<uint8_t> stage(total, 0);
    if (N > 0) { memcpy(&stage[okp], K->keys_un, sizeof(KeyPointRec) * (size_t)N); memcpy(&stage[odesc], K->desc, 32 * (size_t)N); }
    float* ur = (float*)&stage[our];
    for (int i = 0; i < N1; i++) ur[i] = (K->u_right && i < N) ? K->u_right[i] : -1.0f;
    int* nof = (int*)&stage[onof];
    for (int i = 0; i < N1; i++) nof[i] = -1;
    if (nn > 0) {
        memcpy(&stage[onid], K->fv_node_id, 4 * (size_t)nn); memcpy(&stage[ost], K->fv_start, 4 * (size_t)(nn + 1));
        int* ft = (int*)&stage[oft];
        for (int a = 0; a < nn; a++) {
            if (a > 0 && K->fv_node_id[a] <= K->fv_node_id[a - 1]) return fail(ORBX_E_ARG, "feature vector node ids not ascending");
            for (int k = K->fv_start[a]; k < K->fv_start[a + 1]; k++) {
                const int f = (int)K->fv_feat[k];
                if (f < 0 || f >= N) return fail(ORBX_E_ARG, "feature vector entry out of range");
                ft[k] = f; nof[f] = a;
            }
        }
    }
    orbm_keyframe* kf = new orbm_keyframe();
    kf->device = h->device; kf->N = N; kf->fv_nodes = nn; kf->nlevels = K->nlevels;
    kf->dmem = (uint8_t*)rt::dmalloc(total);
    if (!kf->dmem || rt::copy_h2d(kf->dmem, stage.data(), total, h->s0) || rt::stream_sync(h->s0)) { rt::dfree(kf->dmem); delete kf; return fail(ORBX_E_DEVICE, "key frame upload failed"); }
    kf->dev.kps = (const KeyPointRec*)(kf->dmem + okp); kf->dev.desc = (const unsigned long long*)(kf->dmem + odesc); kf->dev.ur = (const float*)(kf->dmem + our);
    kf->dev.node_id = (const uint32_t*)(kf->dmem + onid); kf->dev.fv_start = (const int*)(kf->dmem + ost); kf->dev.fv_feat = (const int*)(kf->dmem + oft);
    kf->dev.node_of_feat = (const int*)(kf->dmem + onof); kf->dev.N = N; kf->dev.fv_nodes = nn;
    kf->angle.resize(N1);
    for (int i = 0; i < N; i++) kf->angle[i] = K->keys_un[i].angle;
    for (int l = 0; l < kMaxLevels; l++) { kf->scale[l] = l < K->nlevels && K->scale_factors ? K->scale_factors[l] : 1.0f; kf->sigma2[l] = l < K->nlevels && K->level_sigma2 ? K->level_sigma2[l] : 1.0f; }
    *out = kf;
    return ORBX_OK;
}

void orbm_keyframe_destroy(orbm_keyframe* kf) {
    if (!kf) return;
    rt::set_device(kf->device);
    rt::dfree(kf->dmem);
    for (KfGrid* g : kf->grids) { rt::dfree(g->mem); delete g; }
    delete kf;
}

// ---- key frames made on the device from frames of the last extraction ----
// recs name where each frame and its FeatureVector sit (source pointers and cap filled in by the entry points, which have refused everything they can
// refuse by then).  k_keyframe_counts tells the host the sizes - one small block down -, the blocks are allocated with the layout of orbm_keyframe_create,
// k_keyframe_snapshot fills all of them in one launch, and the angles come down for the host's copy.  rowcap: most features of one frame.  Blocking.
static int keyframes_from_records(orbx_extractor* h, const char* entry, std::vector<KfSnapRec>& recs, int rowcap, orbm_keyframe** out) {
    const int n = (int)recs.size();
    Packer pk(h);
    const size_t pr = pk.add(recs.data(), sizeof(KfSnapRec) * recs.size()), pc = pk.room(12 * (size_t)n), pa = pk.room(4 * (size_t)n * rowcap);
    if (int e = pk.flush()) return fail(ORBX_E_DEVICE, "%s: %s", entry, upload_error(e));
    ORBX_LAUNCH(k_keyframe_counts, dim3((n + 63) / 64, 1, 1), dim3(64, 1, 1), 0, h->s0, pk.dev<KfSnapRec>(pr), n, pk.out<int>(pc));
    std::vector<int> cnt(3 * (size_t)n);
    if (fetch_sync(h, cnt.data(), pk.dev<int>(pc), 12 * (size_t)n) || rt::check_launch()) return fail(ORBX_E_DEVICE, "%s: reading the frames' sizes failed: %s", entry, rt::last_error());
    int nmax = 1; size_t atotal = 0;
    for (int j = 0; j < n; j++) {
        const int N = cnt[3 * j], nn = cnt[3 * j + 1], nf = cnt[3 * j + 2];
        if (N < 0 || N > rowcap || N >= 65535) return fail(ORBX_E_CAPACITY, "%s: key frame %d would have %d features", entry, j, N);
        if (nn < 0 || nf < nn || nf > N) return fail(ORBX_E_INTERNAL, "%s: key frame %d: a FeatureVector of %d nodes and %d entries does not fit %d features", entry, j, nn, nf, N);
    }
    std::vector<orbm_keyframe*> made(n, nullptr);
    auto drop = [&]() { for (orbm_keyframe* kf : made) if (kf) { rt::dfree(kf->dmem); delete kf; } };
    for (int j = 0; j < n; j++) {
        const int N = cnt[3 * j], N1 = std::max(N, 1), nn = cnt[3 * j + 1], nf = cnt[3 * j + 2];
        const size_t okp = 0, odesc = okp + al16(sizeof(KeyPointRec) * (size_t)N1), our = odesc + al16(32 * (size_t)N1), onid = our + al16(4 * (size_t)N1),
                     ost = onid + al16(4 * (size_t)(nn + 1)), oft = ost + al16(4 * (size_t)(nn + 1)), onof = oft + al16(4 * (size_t)(nf + 1)),
                     total = onof + al16(4 * (size_t)N1);
        orbm_keyframe* kf = made[j] = new orbm_keyframe();
        kf->device = h->device; kf->N = N; kf->fv_nodes = nn; kf->nlevels = h->nlevels;
        kf->dmem = (uint8_t*)rt::dmalloc(total);
        if (!kf->dmem) { drop(); return fail(ORBX_E_DEVICE, "%s: allocating key frame %d failed", entry, j); }
        kf->dev.kps = (const KeyPointRec*)(kf->dmem + okp); kf->dev.desc = (const unsigned long long*)(kf->dmem + odesc); kf->dev.ur = (const float*)(kf->dmem + our);
        kf->dev.node_id = (const uint32_t*)(kf->dmem + onid); kf->dev.fv_start = (const int*)(kf->dmem + ost); kf->dev.fv_feat = (const int*)(kf->dmem + oft);
        kf->dev.node_of_feat = (const int*)(kf->dmem + onof); kf->dev.N = N; kf->dev.fv_nodes = nn;
        for (int l = 0; l < kMaxLevels; l++) { kf->scale[l] = l < h->nlevels ? h->scale[l] : 1.0f; kf->sigma2[l] = l < h->nlevels ? h->sigma2[l] : 1.0f; }
        KfSnapRec& R = recs[j];
        R.dst = kf->dmem; R.angle = pk.out<float>(pa) + atotal;
        R.o_desc = (unsigned)odesc; R.o_ur = (unsigned)our; R.o_nid = (unsigned)onid; R.o_st = (unsigned)ost; R.o_ft = (unsigned)oft; R.o_nof = (unsigned)onof;
        R.N = N; R.nn = nn; R.nf = nf;
        atotal += (size_t)N; nmax = std::max(nmax, N);
    }
    if (int e = pk.flush()) { drop(); return fail(ORBX_E_DEVICE, "%s: %s", entry, upload_error(e)); }
    // a thread moves ~4 dwords of the largest section (7 per keypoint record)
    const int chunks = std::min(16, std::max(1, (7 * nmax + 1023) / 1024));
    ORBX_LAUNCH(k_keyframe_snapshot, dim3(chunks, n, 1), dim3(256, 1, 1), 0, h->s0, pk.dev<KfSnapRec>(pr));
    std::vector<float> angles(std::max<size_t>(atotal, 1));
    if (fetch_sync(h, angles.data(), pk.dev<float>(pa), 4 * atotal) || rt::check_launch()) { drop(); return fail(ORBX_E_DEVICE, "%s: the copy failed: %s", entry, rt::last_error()); }
    size_t a0 = 0;
    for (int j = 0; j < n; j++) {
        orbm_keyframe* kf = made[j];
        kf->angle.assign(std::max(kf->N, 1), 0.0f);
        std::copy(angles.begin() + a0, angles.begin() + a0 + kf->N, kf->angle.begin());
        a0 += (size_t)kf->N;
    }
    for (int j = 0; j < n; j++) out[j] = made[j];
    return ORBX_OK;
}

int orbm_keyframe_create_extracted(orbx_extractor* h, const orbv_vocabulary* v, int n, const int* frames, int use_u_right, orbm_keyframe** out) {
    static const char* const entry = "orbm_keyframe_create_extracted";
    if (!h || n < 0 || (n > 0 && (!frames || !out))) return fail(ORBX_E_ARG, "%s: null argument or n < 0", entry);
    if (n == 0) return ORBX_OK;
    if (n > 65535) return fail(ORBX_E_CAPACITY, "%s: at most 65535 key frames per call", entry);
    if (h->lastB <= 0) return fail(ORBX_E_ARG, "%s: the handle has not extracted anything yet", entry);
    if (undistort_stale(h)) return fail(ORBX_E_ARG, "%s: orbx_set_undistort was called after the last extraction: extract again before making key frames of its frames", entry);
    VocFrameArrays V; memset(&V, 0, sizeof V);
    std::unique_lock<std::mutex> vlk;
    int lo = 0, hi = h->lastB;                                   // the images a key frame may be made of
    if (v) {
        vlk = orbv_lock(v);                                      // until the copy has run: no other handle's run replaces the FeatureVectors under the kernel
        if (orbv_frame_arrays(v, &V)) return fail(ORBX_E_ARG, "%s: run orbv_transform_extracted(v, h, first, B, levelsup) on this extraction first: the FeatureVectors are read where it leaves them", entry);
        if (V.device != h->device) return fail(ORBX_E_ARG, "%s: vocabulary and extractor live on different devices", entry);
        if (V.rig) return fail(ORBX_E_ARG, "%s: the last vocabulary transform was a rig transform (orbv_transform_rig_extracted): make its key frames with orbm_keyframe_create_rig_extracted", entry);
        if (V.handle != (const void*)h || V.cap != h->kp_total_cap || V.first < 0 || V.first + V.lastB > h->lastB)
            return fail(ORBX_E_ARG, "%s: the vocabulary's last transform did not run on this handle, or its results were overwritten: run orbv_transform_extracted on this extraction", entry);
        if (V.extract_gen != h->extract_gen)
            return fail(ORBX_E_ARG, "%s: the handle has extracted another batch since orbv_transform_extracted ran: its FeatureVectors index the keypoints of the previous batch - transform again", entry);
        lo = V.first; hi = V.first + V.lastB;
    }
    for (int j = 0; j < n; j++) {
        if (frames[j] < lo || frames[j] >= hi)
            return fail(ORBX_E_ARG, v ? "%s: key frame %d names image %d, the vocabulary transform covers [%d, %d)" : "%s: key frame %d names image %d, the last extraction holds [%d, %d)", entry, j, frames[j], lo, hi);
        if (use_u_right && (h->ur_B <= 0 || h->ur_gen != h->extract_gen || frames[j] < h->ur_first || frames[j] >= h->ur_first + h->ur_B))
            return fail(ORBX_E_ARG, "%s: use_u_right, but image %d has no results of orbm_stereo_match / orbm_stereo_from_depth on this extraction", entry, frames[j]);
    }
    rt::set_device(h->device);
    const int cap = h->kp_total_cap;
    std::vector<KfSnapRec> recs(n);
    for (int j = 0; j < n; j++) {
        const size_t f = (size_t)frames[j];
        KfSnapRec& R = recs[j]; memset(&R, 0, sizeof R);
        R.kps = (h->ex_undist_active ? h->d_kps_un.p : h->d_kps.p) + f * cap;                        // mvKeysUn
        R.n_l = h->d_nm.p + f; R.desc = h->d_desc.p + f * cap * 4; R.cap = cap;
        if (use_u_right) R.ur = h->d_uRight.p + (f - (size_t)h->ur_first) * cap;
        if (v) {
            const size_t b = f - (size_t)V.first;
            R.node_id = V.fv_node + b * cap; R.fv_start = V.fv_start + b * (cap + 1); R.fv_feat = V.fv_feat + b * cap; R.fv_nodes = V.nout + 2 * b + 1;
        }
    }
    return keyframes_from_records(h, entry, recs, cap, out);
}

int orbm_keyframe_create_rig_extracted(orbx_extractor* L, int lf, orbx_extractor* R, int rf, const orbv_vocabulary* v, int n, const int* frames, orbm_keyframe** out) {
    static const char* const entry = "orbm_keyframe_create_rig_extracted";
    if (!L || !R || !v || n < 0 || (n > 0 && (!frames || !out))) return fail(ORBX_E_ARG, "%s: null argument or n < 0", entry);
    if (n == 0) return ORBX_OK;
    if (n > 65535) return fail(ORBX_E_CAPACITY, "%s: at most 65535 key frames per call", entry);
    if (L->lastB <= 0 || R->lastB <= 0) return fail(ORBX_E_ARG, "%s: a handle has not extracted anything yet", entry);
    VocFrameArrays V;
    const std::unique_lock<std::mutex> vlk = orbv_lock(v);       // as in orbm_keyframe_create_extracted
    if (orbv_frame_arrays(v, &V) || !V.rig)
        return fail(ORBX_E_ARG, "%s: no rig transform: run orbv_transform_rig_extracted(v, L, %d, R, %d, B, levelsup) first - the rig frames' rows and FeatureVectors are read where it leaves them", entry, lf, rf);
    if (V.handle != (const void*)L || V.handle_r != (const void*)R || V.first != lf || V.first_r != rf)
        return fail(ORBX_E_ARG, "%s: the last rig transform covered other handles or frames (left %d, right %d, %d frames)", entry, V.first, V.first_r, V.lastB);
    if (V.extract_gen != L->extract_gen || V.extract_gen_r != R->extract_gen)
        return fail(ORBX_E_ARG, "%s: a handle has extracted since orbv_transform_rig_extracted ran: its FeatureVectors index the keypoints of the previous batch - transform again", entry);
    if (V.device != L->device || R->device != L->device) return fail(ORBX_E_ARG, "%s: vocabulary and extractors live on different devices", entry);
    const int cap = L->kp_total_cap, S = V.cap, B = V.lastB;
    if (S != 2 * cap || R->kp_total_cap != cap || lf < 0 || rf < 0 || lf + B > L->lastB || rf + B > R->lastB) return fail(ORBX_E_ARG, "%s: the rig transform does not match the handles' extractions", entry);
    for (int j = 0; j < n; j++)
        if (frames[j] < 0 || frames[j] >= B) return fail(ORBX_E_ARG, "%s: key frame %d names frame %d, the rig transform holds %d", entry, j, frames[j], B);
    rt::set_device(L->device);
    if (L != R) { record_done_if_pending(R); rt::stream_wait_event(L->s0, R->ev_done); }          // R's extraction runs on R's stream
    std::vector<KfSnapRec> recs(n);
    for (int j = 0; j < n; j++) {
        const size_t b = (size_t)frames[j];
        KfSnapRec& Q = recs[j]; memset(&Q, 0, sizeof Q);
        Q.kps = L->d_kps.p + ((size_t)lf + b) * cap; Q.kps_r = R->d_kps.p + ((size_t)rf + b) * cap;   // mvKeys, mvKeysRight
        Q.n_l = L->d_nm.p + lf + b; Q.n_r = R->d_nm.p + rf + b; Q.cap = cap;
        Q.desc = V.desc + b * S * 4;
        Q.node_id = V.fv_node + b * S; Q.fv_start = V.fv_start + b * (S + 1); Q.fv_feat = V.fv_feat + b * S; Q.fv_nodes = V.nout + 2 * b + 1;
    }
    return keyframes_from_records(L, entry, recs, S, out);
}

int orbm_keyframe_fetch(orbx_extractor* h, const orbm_keyframe* kf, int* N, int* fv_nodes, OrbxKeyPoint* keys_un, uint8_t* desc, float* u_right, uint32_t* fv_node,
                        int* fv_start, uint32_t* fv_feat, int* node_of_feat) {
    if (!h || !kf) return fail(ORBX_E_ARG, "orbm_keyframe_fetch: null handle or key frame");
    if (kf->device != h->device) return fail(ORBX_E_ARG, "orbm_keyframe_fetch: the key frame lives on another device");
    rt::set_device(h->device);
    if (N) *N = kf->N;
    if (fv_nodes) *fv_nodes = kf->fv_nodes;
    const size_t n = (size_t)kf->N, nn = (size_t)kf->fv_nodes;
    // the sections are contiguous: everything from the keypoints to the feature indices' end comes down in one copy
    const uint8_t* base = kf->dmem;
    const size_t o_st = (const uint8_t*)kf->dev.fv_start - base, o_ft = (const uint8_t*)kf->dev.fv_feat - base, o_nof = (const uint8_t*)kf->dev.node_of_feat - base;
    const size_t total = o_nof + 4 * std::max<size_t>(n, 1);
    std::vector<uint8_t> img(total);
    if (fetch_sync(h, img.data(), base, total)) return fail(ORBX_E_DEVICE, "orbm_keyframe_fetch: D2H failed: %s", rt::last_error());
    if (keys_un && n) memcpy(keys_un, img.data(), sizeof(KeyPointRec) * n);
    if (desc && n) memcpy(desc, img.data() + ((const uint8_t*)kf->dev.desc - base), 32 * n);
    if (u_right && n) memcpy(u_right, img.data() + ((const uint8_t*)kf->dev.ur - base), 4 * n);
    if (fv_node && nn) memcpy(fv_node, img.data() + ((const uint8_t*)kf->dev.node_id - base), 4 * nn);
    const int* st = (const int*)(img.data() + o_st);
    if (fv_start) memcpy(fv_start, st, 4 * (nn + 1));
    if (fv_feat && nn && st[nn] > 0) memcpy(fv_feat, img.data() + o_ft, 4 * (size_t)st[nn]);
    if (node_of_feat && n) memcpy(node_of_feat, img.data() + o_nof, 4 * n);
    return ORBX_OK;
}

// rotation-consistency pruning shared by the resident searches: m12 entries outside the three strongest bins of the angle-difference
// histogram are reset (src/ORBmatcher.cc:1270-1286); returns the number of matches left
static int prune_by_rotation(const orbm_keyframe* K1, const orbm_keyframe* K2, int* m12, bool check_ori) {
    int nmatches = 0;
    RotHist hist;
    for (int i = 0; i < K1->N; i++) {
        if (m12[i] < 0) continue;
        nmatches++;
        if (check_ori) hist.add(K1->angle[i], K2->angle[m12[i]], i);
    }
    if (check_ori) hist.prune([&](int idx1) { m12[idx1] = -1; nmatches--; });
    return nmatches;
}

// The call-time flag block of a resident search: every flag array of the call, 16-byte aligned, one behind the other in the order the search documents, and where
// the arrays come from - the caller's own arrays (host-fed: arrays[list][i], nullptr: none) or the key frames' rows in an orbm_map (map-fed: rows[list][i], -1: none;
// the .._map entry points at the end of this file have checked the rows and hold the map's mutex until the call returns).  A search has at most two lists of arrays.
// add() hands out the offsets, pack() puts the block behind the call's records in the one upload - the bytes themselves (host-fed), or the records of
// k_map_row_flags and room for the block (map-fed: room() has to follow the last add()) - and fill(), after flush(), writes a map-fed block in ONE launch, each
// array at the offset the host-fed call uploads it at.  The block is never shorter than 16 bytes; what lies between the arrays is not read.
struct CallFlags {
    const uint8_t* const* arrays[2]; const int* rows[2];
    const int* kf_slots; int row_cap; const uint8_t* state;                 // the map's rows and slot states (kf_slots == nullptr: host-fed)
    struct Piece { const uint8_t* src; int n, off; };
    std::vector<Piece> pieces; std::vector<MapRowFlagRec> recs; std::vector<uint8_t> bytes;
    size_t total = 0, pf = 0, pr = 0;
    CallFlags(const uint8_t* const* a0, const uint8_t* const* a1) : arrays{a0, a1}, rows{nullptr, nullptr}, kf_slots(nullptr), row_cap(0), state(nullptr) {}
    CallFlags(const int* slots, int cap, const uint8_t* st, const int* r0, const int* r1) : arrays{nullptr, nullptr}, rows{r0, r1}, kf_slots(slots), row_cap(cap), state(st) {}
    // the offset of array i of a list, n flags long, or -1: no array was passed, or the key frame has no features.  always: the search reads the array
    // unconditionally - it gets an offset (and at least 16 bytes) even then, all zero where the caller passed none
    int add(int list, int i, int n, int rule, bool always = false) {
        const uint8_t* src = arrays[list] ? arrays[list][i] : nullptr;
        const int row = rows[list] ? rows[list][i] : -1;
        const bool given = n > 0 && (kf_slots ? row >= 0 : src != nullptr);
        if (!given && !always) return -1;
        const int off = (int)total;
        total += al16((size_t)std::max(n, 1));
        if (given && kf_slots) recs.push_back({row, n, off, rule});
        else if (given) pieces.push_back({src, n, off});
        return off;
    }
    void pack(Packer& pk) {
        const size_t block = std::max<size_t>(total, 16);
        if (kf_slots) { pr = pk.add(recs.data(), sizeof(MapRowFlagRec) * recs.size()); pf = pk.room(block); return; }
        bytes.assign(block, 0);
        for (const Piece& p : pieces) memcpy(&bytes[p.off], p.src, (size_t)p.n);
        pf = pk.add(bytes.data(), bytes.size());
    }
    void fill(orbx_extractor* h, const Packer& pk) const {
        int longest = 0;
        for (const MapRowFlagRec& r : recs) longest = std::max(longest, r.n);
        if (longest <= 0) return;                                            // host-fed, or no array of the call holds a flag
        const dim3 grid((longest + 255) / 256, (unsigned)recs.size(), 1), blk(256, 1, 1);
        const int* slots = kf_slots; const int cap = row_cap; const uint8_t* st = state;
        const MapRowFlagRec* d_recs = pk.dev<MapRowFlagRec>(pr); uint8_t* d_flags = pk.out<uint8_t>(pf);
        ORBX_LAUNCH(k_map_row_flags, grid, blk, 0, h->s0, slots, cap, st, d_recs, d_flags);
    }
    const uint8_t* dev(const Packer& pk) const { return pk.dev<uint8_t>(pf); }
};

// flags: list 0 holds has_map_point1 (one array), list 1 has_map_point2 of neighbour j; from a map under the rule "holds a point"
static int sft_resident_impl(orbx_extractor* h, orbm_keyframe* K1, CallFlags flags, int n2, orbm_keyframe* const* K2s, const float* F12s, const OrbmKB8Pair* kb8,
                             const float* eps, int only_stereo, int coarse, int check_ori, int* matches12, int* nmatches_out) {
    if (!h || !K1 || n2 < 0 || (n2 > 0 && (!K2s || (!F12s && !kb8) || !eps || !matches12))) return fail(ORBX_E_ARG, "null");
    if (K1->device != h->device) return fail(ORBX_E_ARG, "key frame lives on another device");
    rt::set_device(h->device);
    const int N1 = K1->N;
    if (n2 == 0 || N1 == 0) { for (int j = 0; j < n2; j++) if (nmatches_out) nmatches_out[j] = 0; return ORBX_OK; }
    // call-time flags: KF1's map point flags at 0, then each neighbour's (the kernel reads them all: an array that was not passed is all zero)
    flags.add(0, 0, N1, kRowHoldsPoint, true);
    std::vector<SftNeighbour> nb(n2);
    for (int j = 0; j < n2; j++) {
        const orbm_keyframe* K2 = K2s[j];
        if (!K2 || K2->device != h->device) return fail(ORBX_E_ARG, "bad neighbour key frame %d", j);
        SftNeighbour& S = nb[j]; memset(&S, 0, sizeof S);
        S.k2 = K2->dev; S.mp2_off = flags.add(1, j, K2->N, kRowHoldsPoint, true);
        BowParams& P = S.P;
        if (F12s) for (int i = 0; i < 9; i++) P.F12[i] = F12s[9 * (size_t)j + i];
        P.ep[0] = eps[2 * (size_t)j]; P.ep[1] = eps[2 * (size_t)j + 1];
        for (int l = 0; l < kMaxLevels; l++) { P.scale2[l] = K2->scale[l]; P.sigma2_2[l] = K2->sigma2[l]; }
        P.only_stereo = only_stereo; P.coarse = coarse; P.th_low = TH_LOW; P.nleft1 = P.nleft2 = -1;
        if (kb8) fill_kb8(P, kb8[j], K1->sigma2, kMaxLevels);                // Kannala-Brandt cameras: one OrbmKB8Pair per neighbour (as orbm_search_for_triangulation_kb8)
    }
    Packer pk(h);
    const size_t pn = pk.add(nb.data(), sizeof(SftNeighbour) * nb.size());
    flags.pack(pk);
    if (pk.flush() || h->d_si[SI_BEST].ensure((size_t)n2 * N1)) return fail(ORBX_E_DEVICE, "upload/allocation failed");
    flags.fill(h, pk);
    dim3 grid((N1 + 3) / 4, n2, 1), blk(256, 1, 1);
    if (kb8) ORBX_LAUNCH(k_sft_resident_kb8, grid, blk, 0, h->s0, K1->dev, flags.dev(pk), pk.dev<SftNeighbour>(pn), h->d_si[SI_BEST].p);
    else ORBX_LAUNCH(k_sft_resident, grid, blk, 0, h->s0, K1->dev, flags.dev(pk), pk.dev<SftNeighbour>(pn), h->d_si[SI_BEST].p);
    if (fetch_sync(h, matches12, h->d_si[SI_BEST].p, sizeof(int) * (size_t)n2 * N1) || rt::check_launch())
        return fail(ORBX_E_DEVICE, "resident triangulation search failed: %s", rt::last_error());
    for (int j = 0; j < n2; j++) {
        const int nm = prune_by_rotation(K1, K2s[j], matches12 + (size_t)j * N1, check_ori != 0);
        if (nmatches_out) nmatches_out[j] = nm;
    }
    return ORBX_OK;
}

int orbm_search_for_triangulation_resident(orbx_extractor* h, orbm_keyframe* K1, const uint8_t* has_mp1, int n2, orbm_keyframe* const* K2s,
                                           const uint8_t* const* has_mp2, const float* F12s, const float* eps, int only_stereo, int coarse, int check_ori,
                                           int* matches12, int* nmatches_out) {
    if (n2 > 0 && !F12s) return fail(ORBX_E_ARG, "null");
    return sft_resident_impl(h, K1, CallFlags(&has_mp1, has_mp2), n2, K2s, F12s, nullptr, eps, only_stereo, coarse, check_ori, matches12, nmatches_out);
}

int orbm_search_for_triangulation_resident_kb8(orbx_extractor* h, orbm_keyframe* K1, const uint8_t* has_mp1, int n2, orbm_keyframe* const* K2s,
                                               const uint8_t* const* has_mp2, const OrbmKB8Pair* cams, const float* eps, int only_stereo, int coarse, int check_ori,
                                               int* matches12, int* nmatches_out) {
    if (n2 > 0 && !cams) return fail(ORBX_E_ARG, "null");
    return sft_resident_impl(h, K1, CallFlags(&has_mp1, has_mp2), n2, K2s, nullptr, cams, eps, only_stereo, coarse, check_ori, matches12, nmatches_out);
}

// The result block of the resident BoW searches in d_si[SI_BEST]: nout results, pre-set to -1 | 4 status words | `extra` counts, both zeroed.  ensure() goes
// with the upload, clear() in front of the search's launches, fetch() behind them: ONE copy brings the whole block down into res
struct BowResults {
    orbx_extractor* h; size_t nout, extra; std::vector<int> res;
    size_t total() const { return nout + 4 + extra; }
    int* dev() const { return h->d_si[SI_BEST].p; }
    int* status() const { return dev() + nout; }
    int* counts() const { return dev() + nout + 4; }
    bool ensure() const { return h->d_si[SI_BEST].ensure(total()) != 0; }
    int clear() const {
        if (rt::memset_async(dev(), 0xFF, sizeof(int) * nout, h->s0) || rt::memset_async(status(), 0, sizeof(int) * (4 + extra), h->s0)) return fail(ORBX_E_DEVICE, "memset failed");
        return ORBX_OK;
    }
    // search: names the call in a failure's text; k2: what the second side of a pair is, for the refusal of an overfull vocabulary node (status bit 4)
    int fetch(const char* search, const char* k2) {
        res.resize(total());
        if (fetch_sync(h, res.data(), dev(), sizeof(int) * total()) || rt::check_launch()) return fail(ORBX_E_DEVICE, "%s failed: %s", search, rt::last_error());
        if (res[nout] & 4) return fail(ORBX_E_CAPACITY, "a vocabulary node holds more than 2048 features of one %s", k2);
        return ORBX_OK;
    }
};

// frame b of a vocabulary transform as the second key frame of a BoW pair: its FeatureVector where the transform left it, in rows of `width` entries (the
// extractor's capacity, twice that for a rig frame); the node count is read on the device (BowPairResident::k2_nodes_dev)
static ResidentKF frame_as_k2(const VocFrameArrays& V, int b, int width, const KeyPointRec* kps, const unsigned long long* desc) {
    ResidentKF K; memset(&K, 0, sizeof K);
    K.kps = kps; K.desc = desc;
    K.node_id = V.fv_node + (size_t)b * width; K.fv_start = V.fv_start + (size_t)b * (width + 1); K.fv_feat = V.fv_feat + (size_t)b * width;
    K.N = width;
    return K;
}

// flags: list 0 holds has_map_point1 of pair p, list 1 eligible2 (none: every feature is eligible); from a map under the rule "holds a good point"
static int bow_resident_impl(orbx_extractor* h, int n, orbm_keyframe* const* K1s, orbm_keyframe* const* K2s, CallFlags flags, float nnratio, int th_inclusive,
                             int check_ori, int* const* matches12, int* nmatches_out) {
    if (!h || n < 0 || (n > 0 && (!K1s || !K2s || !matches12))) return fail(ORBX_E_ARG, "null");
    rt::set_device(h->device);
    if (n == 0) return ORBX_OK;
    int N1cap = 1, maxnodes = 1;
    std::vector<BowPairResident> pairs(n);
    for (int p = 0; p < n; p++) {
        const orbm_keyframe *K1 = K1s[p], *K2 = K2s[p];
        if (!K1 || !K2 || !matches12[p] || K1->device != h->device || K2->device != h->device) return fail(ORBX_E_ARG, "bad key frame pair %d", p);
        BowPairResident& B = pairs[p];
        B.k1 = K1->dev; B.k2 = K2->dev; B.k2_nodes_dev = nullptr;
        B.mp1_off = flags.add(0, p, K1->N, kRowHoldsGoodPoint); B.elig2_off = flags.add(1, p, K2->N, kRowHoldsGoodPoint);
        N1cap = std::max(N1cap, K1->N); maxnodes = std::max(maxnodes, K1->fv_nodes);
    }
    Packer pk(h);
    const size_t pp = pk.add(pairs.data(), sizeof(BowPairResident) * pairs.size());
    flags.pack(pk);
    BowResults R = {h, (size_t)n * N1cap, 0, {}};
    if (pk.flush() || R.ensure()) return fail(ORBX_E_DEVICE, "upload/allocation failed");
    flags.fill(h, pk);
    if (int rc = R.clear()) return rc;
    dim3 grid((maxnodes + 3) / 4, n, 1), blk(256, 1, 1);
    ORBX_LAUNCH(k_bow_match_resident, grid, blk, 0, h->s0, pk.dev<BowPairResident>(pp), flags.dev(pk), nnratio, TH_LOW, th_inclusive, R.dev(), N1cap, R.status());
    if (int rc = R.fetch("resident bow search", "key frame")) return rc;
    for (int p = 0; p < n; p++) {
        const int N1 = K1s[p]->N;
        if (N1 > 0) memcpy(matches12[p], &R.res[(size_t)p * N1cap], sizeof(int) * (size_t)N1);
        const int nm = prune_by_rotation(K1s[p], K2s[p], matches12[p], check_ori != 0);
        if (nmatches_out) nmatches_out[p] = nm;
    }
    return ORBX_OK;
}

int orbm_search_by_bow_resident(orbx_extractor* h, int n, orbm_keyframe* const* K1s, const uint8_t* const* has_mp1, orbm_keyframe* const* K2s,
                                const uint8_t* const* eligible2, float nnratio, int th_inclusive, int check_ori, int* const* matches12, int* nmatches_out) {
    return bow_resident_impl(h, n, K1s, K2s, CallFlags(has_mp1, eligible2), nnratio, th_inclusive, check_ori, matches12, nmatches_out);
}

// ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches) (src/ORBmatcher.cc:259-493) for the frames of a batch: frame b of the last
// extraction (its FeatureVector where orbv_transform_extracted left it) against the resident key frame KFs[b].  Two launches for the whole batch:
// k_bow_match_resident (the accept loop per vocabulary node) and k_bow_rotation_prune (histogram, three maxima, resets, counts) - nothing but the
// call-time flags goes up, nothing but the matches comes down.  The caller holds the vocabulary's lock until the matches are down: no other handle's run
// replaces the FeatureVectors under the kernels.  flags: list 0 holds has_map_point1 of frame b's key frame - the caller's arrays or, filled on the device,
// the key frames' rows in a map whose mutex the caller holds as well (rule "holds a good point").
static int bow_frames_batch_locked(orbx_extractor* h, const orbv_vocabulary* v, int first, int B, orbm_keyframe* const* KFs, CallFlags flags, float nnratio,
                                   int check_ori, int* const* matches12, int* nmatches_out) {
    VocFrameArrays V;
    if (orbv_frame_arrays(v, &V) == 0 && V.rig)
        return fail(ORBX_E_ARG, "the last vocabulary transform was a rig transform (orbv_transform_rig_extracted): search its frames with orbm_search_by_bow_rig_batch");
    if (orbv_frame_arrays(v, &V) || V.handle != (const void*)h || V.first != first || V.lastB != B || V.cap != h->kp_total_cap || first < 0 || first + B > h->lastB)
        return fail(ORBX_E_ARG, "run orbv_transform_extracted(v, h, %d, %d, levelsup) on this extraction first: the FeatureVectors of these frames are read where it leaves them", first, B);
    if (V.extract_gen != h->extract_gen)
        return fail(ORBX_E_ARG, "the handle has extracted another batch since orbv_transform_extracted ran: its FeatureVectors index the keypoints of the previous batch - transform again");
    if (V.device != h->device) return fail(ORBX_E_ARG, "vocabulary and extractor live on different devices");
    if (undistort_stale(h)) return fail(ORBX_E_ARG, "orbx_set_undistort was called after the last extraction: extract again before searching its frames");
    rt::set_device(h->device);
    const int cap = h->kp_total_cap;
    int N1cap = 1, maxnodes = 1;
    std::vector<BowPairResident> pairs(B);
    for (int b = 0; b < B; b++) {
        const orbm_keyframe* K1 = KFs[b];
        if (!K1 || !matches12[b] || K1->device != h->device) return fail(ORBX_E_ARG, "bad key frame of frame %d", b);
        BowPairResident& P = pairs[b];
        memset(&P, 0, sizeof P);
        P.k1 = K1->dev;
        P.k2 = frame_as_k2(V, b, cap, (h->ex_undist_active ? h->d_kps_un.p : h->d_kps.p) + (size_t)(first + b) * cap,      // F.mvKeysUn (the angle is what is read of it)
                           h->d_desc.p + (size_t)(first + b) * cap * 4);
        P.k2_nodes_dev = V.nout + 2 * b + 1;
        P.mp1_off = flags.add(0, b, K1->N, kRowHoldsGoodPoint); P.elig2_off = -1;
        N1cap = std::max(N1cap, K1->N); maxnodes = std::max(maxnodes, K1->fv_nodes);
    }
    Packer pk(h);
    const size_t pp = pk.add(pairs.data(), sizeof(BowPairResident) * pairs.size());
    flags.pack(pk);
    BowResults R = {h, (size_t)B * N1cap, (size_t)B, {}};                          // matches | status | nmatches
    if (pk.flush() || R.ensure()) return fail(ORBX_E_DEVICE, "upload/allocation failed");
    flags.fill(h, pk);
    if (int rc = R.clear()) return rc;
    if (h->profile) rt::event_record(h->ev_stage[ST_MATCH][0], h->s0);
    dim3 grid((maxnodes + 3) / 4, B, 1), blk(256, 1, 1);
    ORBX_LAUNCH(k_bow_match_resident, grid, blk, 0, h->s0, pk.dev<BowPairResident>(pp), flags.dev(pk), nnratio, TH_LOW, 1, R.dev(), N1cap, R.status());
    dim3 gridp(B, 1, 1), blkp(64, 1, 1);
    ORBX_LAUNCH(k_bow_rotation_prune, gridp, blkp, 0, h->s0, pk.dev<BowPairResident>(pp), R.dev(), N1cap, check_ori, R.counts());
    if (h->profile) rt::event_record(h->ev_stage[ST_MATCH][1], h->s0);
    if (int rc = R.fetch("batched bow search", "frame")) return rc;
    for (int b = 0; b < B; b++) {
        const int N1 = KFs[b]->N;
        if (N1 > 0) memcpy(matches12[b], &R.res[(size_t)b * N1cap], sizeof(int) * (size_t)N1);
        if (nmatches_out) nmatches_out[b] = R.res[R.nout + 4 + b];
    }
    return ORBX_OK;
}

int orbm_search_by_bow_frames_batch(orbx_extractor* h, const orbv_vocabulary* v, int first, int B, orbm_keyframe* const* KFs, const uint8_t* const* has_mp1,
                                    float nnratio, int check_ori, int* const* matches12, int* nmatches_out) {
    if (!h || !v || B <= 0 || !KFs || !has_mp1 || !matches12) return fail(ORBX_E_ARG, "null");
    const std::unique_lock<std::mutex> vlk = orbv_lock(v);
    return bow_frames_batch_locked(h, v, first, B, KFs, CallFlags(has_mp1, nullptr), nnratio, check_ori, matches12, nmatches_out);
}

// SearchByBoW(pKF, F) for rig frames (F.Nleft != -1, src/ORBmatcher.cc:259-493 incl. :343-372 and :414-446), P (frame, key frame) pairs: rig frame
// frame[p] of the last orbv_transform_rig_extracted(v, L, lf, R, rf, B, .) - its rows and FeatureVector where the transform left them, camera 1's
// keypoints in L, camera 2's in R - against the resident key frame KFs[p].  k_bow_match_rig (the two-camera accept loop per vocabulary node) and
// k_bow_rotation_prune_rig (one histogram over both cameras' matches) for all pairs; assigned[p] is frame-indexed, as orbm_search_by_bow_fisheye's.
// The caller holds the vocabulary's lock (as in orbm_search_by_bow_frames_batch) and has checked its pointers.  flags: list 0 holds has_map_point of pair
// p's key frame; from a map under the rule "holds a good point" (the caller holds the map's mutex as well)
static int bow_rig_batch_locked(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const orbv_vocabulary* v, int P, const int* frame,
                                orbm_keyframe* const* KFs, CallFlags flags, float nnratio, int check_ori, int* const* assigned, int* nmatches_out) {
    VocFrameArrays V;
    if (orbv_frame_arrays(v, &V) || !V.rig)
        return fail(ORBX_E_ARG, "no rig transform: run orbv_transform_rig_extracted(v, L, %d, R, %d, %d, levelsup) first - the rig frames' rows and FeatureVectors are read where it leaves them",
                    lf, rf, B);
    if (V.handle != (const void*)L || V.handle_r != (const void*)R || V.first != lf || V.first_r != rf || V.lastB != B)
        return fail(ORBX_E_ARG, "the last rig transform covered other handles or frames (left %d, right %d, %d frames)", V.first, V.first_r, V.lastB);
    if (V.extract_gen != L->extract_gen || V.extract_gen_r != R->extract_gen)
        return fail(ORBX_E_ARG, "a handle has extracted since orbv_transform_rig_extracted ran: its FeatureVectors index the keypoints of the previous batch - transform again");
    if (V.device != L->device || R->device != L->device) return fail(ORBX_E_ARG, "vocabulary and extractors live on different devices");
    const int cap = L->kp_total_cap, S = V.cap;
    if (S != 2 * cap || lf + B > L->lastB || rf + B > R->lastB) return fail(ORBX_E_ARG, "the rig transform does not match the handles' extractions");
    rt::set_device(L->device);
    int maxnodes = 1;
    std::vector<BowPairRig> pairs(P);
    for (int p = 0; p < P; p++) {
        const int b = frame[p];
        if (b < 0 || b >= B) return fail(ORBX_E_ARG, "pair %d names frame %d, the rig transform holds %d", p, b, B);
        const orbm_keyframe* K = KFs[p];
        if (!K || !assigned[p]) return fail(ORBX_E_ARG, "pair %d: null key frame or output row", p);
        if (K->device != L->device) return fail(ORBX_E_ARG, "pair %d: the key frame lives on another device", p);
        BowPairRig& Q = pairs[p];
        memset(&Q, 0, sizeof Q);
        BowPairResident& M = Q.m;
        M.k1 = K->dev;
        M.k2 = frame_as_k2(V, b, S, L->d_kps.p + (size_t)(lf + b) * cap, V.desc + (size_t)b * S * 4);   // mvKeys; camera 2's mvKeysRight below
        M.k2_nodes_dev = V.nout + 2 * b + 1;
        M.mp1_off = flags.add(0, p, K->N, kRowHoldsGoodPoint); M.elig2_off = -1;
        Q.kps_r = R->d_kps.p + (size_t)(rf + b) * cap;
        Q.nleft = L->d_nm.p + lf + b;
        maxnodes = std::max(maxnodes, K->fv_nodes);
    }
    Packer pk(L);
    const size_t pp = pk.add(pairs.data(), sizeof(BowPairRig) * pairs.size());
    flags.pack(pk);
    BowResults out = {L, (size_t)P * S, (size_t)P, {}};                             // assigned | status | nmatches
    if (pk.flush() || out.ensure()) return fail(ORBX_E_DEVICE, "upload/allocation failed");
    flags.fill(L, pk);
    if (int rc = out.clear()) return rc;
    if (L->profile) rt::event_record(L->ev_stage[ST_MATCH][0], L->s0);
    dim3 grid((maxnodes + 3) / 4, P, 1), blk(256, 1, 1);
    ORBX_LAUNCH(k_bow_match_rig, grid, blk, 0, L->s0, pk.dev<BowPairRig>(pp), flags.dev(pk), nnratio, TH_LOW, out.dev(), S, out.status());
    dim3 gridp(P, 1, 1), blkp(64, 1, 1);
    ORBX_LAUNCH(k_bow_rotation_prune_rig, gridp, blkp, 0, L->s0, pk.dev<BowPairRig>(pp), out.dev(), S, check_ori, out.counts());
    if (L->profile) rt::event_record(L->ev_stage[ST_MATCH][1], L->s0);
    if (int rc = out.fetch("batched rig bow search", "rig frame")) return rc;
    for (int p = 0; p < P; p++) {
        memcpy(assigned[p], &out.res[(size_t)p * S], sizeof(int) * (size_t)S);
        if (nmatches_out) nmatches_out[p] = out.res[out.nout + 4 + p];
    }
    return ORBX_OK;
}

int orbm_search_by_bow_rig_batch(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const orbv_vocabulary* v, int P, const int* frame,
                                 orbm_keyframe* const* KFs, const uint8_t* const* has_map_point, float nnratio, int check_ori, int* const* assigned,
                                 int* nmatches_out) {
    if (!L || !R || !v || B <= 0 || P <= 0 || !frame || !KFs || !has_map_point || !assigned) return fail(ORBX_E_ARG, "null");
    const std::unique_lock<std::mutex> vlk = orbv_lock(v);       // as in orbm_search_by_bow_frames_batch
    return bow_rig_batch_locked(L, lf, R, rf, B, v, P, frame, KFs, CallFlags(has_map_point, nullptr), nnratio, check_ori, assigned, nmatches_out);
}

int orbm_search_by_bow(orbx_extractor* h, const OrbmKeyFrameView* K1, const OrbmKeyFrameView* K2, float nnratio, int th_inclusive,
                       int check_ori, int* matches12, int* nmatches_out) {
    if (!h || !K1 || !K2 || !matches12) return fail(ORBX_E_ARG, "null");
    int nm = 0;
    const int rc = orbm_search_by_bow_batch(h, 1, &K1, &K2, nnratio, th_inclusive, check_ori, &matches12, &nm);
    if (nmatches_out) *nmatches_out = nm;
    return rc;
}

// ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) for a fisheye-rig frame (F.Nleft != -1, src/ORBmatcher.cc:259-493 incl.
// :343-372 and :414-446): best / second best are kept separately for the features of camera 1 (index < nleft2) and of camera 2, the
// camera-2 match is only considered when the camera-1 best passed TH_LOW (:378, :414 nest that way) and takes no ratio test (":417 || true").
// assigned2[j] = feature of K1 whose map point goes to vpMapPointMatches[j], or -1.
int orbm_search_by_bow_fisheye(orbx_extractor* h, const OrbmKeyFrameView* K1, const OrbmKeyFrameView* K2, int nleft2, float nnratio, int check_ori,
                               int* assigned2, int* nmatches_out) {
    if (!h || !K1 || !K2 || !assigned2) return fail(ORBX_E_ARG, "null");
    if (K1->N >= 65535 || K2->N >= 65535 || nleft2 < 0 || nleft2 > K2->N) return fail(ORBX_E_ARG, "bad key frame / frame sizes");
    rt::set_device(h->device);
    const int N1 = K1->N, N2 = K2->N;
    for (int i = 0; i < N2; i++) assigned2[i] = -1;
    std::vector<BowItem> items;
    int total = 0;
    for_each_common_node(K1, K2, [&](int a, int b) {
        for (int k = K1->fv_start[a]; k < K1->fv_start[a + 1]; k++) {
            const int idx1 = (int)K1->fv_feat[k];
            if (!K1->has_map_point || !K1->has_map_point[idx1]) continue;     // !pMP || pMP->isBad()
            BowItem it; it.idx1 = idx1; it.start2 = K2->fv_start[b]; it.cnt2 = K2->fv_start[b + 1] - K2->fv_start[b]; it.out_off = total;
            total += it.cnt2;
            items.push_back(it);
        }
    });
    int nmatches = 0;
    if (!items.empty() && total > 0) {
        std::vector<uint8_t> elig(N2 > 0 ? N2 : 1, 1);
        const int nfeat2 = K2->fv_start[K2->fv_nodes];
        Packer pk(h);
        const size_t pd1 = pk.add(K1->desc, 32 * (size_t)N1), pd2 = pk.add(K2->desc, 32 * (size_t)N2), pel = pk.add(elig.data(), elig.size()),
                     pit = pk.add(items.data(), sizeof(BowItem) * items.size()), pf2 = pk.add(K2->fv_feat, sizeof(int) * (size_t)nfeat2);
        if (pk.flush() || h->d_si[SI_BEST].ensure((size_t)total + 1)) return fail(ORBX_E_DEVICE, "upload/allocation failed");
        dim3 grid(((int)items.size() + 3) / 4, 1, 1), blk(256, 1, 1);
        ORBX_LAUNCH(k_bow_dists, grid, blk, 0, h->s0, pk.dev<BowItem>(pit), (int)items.size(), pk.dev<unsigned long long>(pd1), pk.dev<unsigned long long>(pd2),
                    pk.dev<uint8_t>(pel), pk.dev<int>(pf2), h->d_si[SI_BEST].p);
        std::vector<int> dist((size_t)total);
        if (fetch_sync(h, dist.data(), h->d_si[SI_BEST].p, sizeof(int) * (size_t)total) || rt::check_launch())
            return fail(ORBX_E_DEVICE, "bow distances failed: %s", rt::last_error());
        RotHist hist;
        for (const BowItem& it : items) {
            int bestDist1 = 256, bestIdxF = -1, bestDist2 = 256, bestDist1R = 256, bestIdxFR = -1, bestDist2R = 256;
            for (int j = 0; j < it.cnt2; j++) {
                const int idx2 = (int)K2->fv_feat[it.start2 + j];
                const int d = dist[(size_t)it.out_off + j];
                if (assigned2[idx2] >= 0) continue;                               // vpMapPointMatches[realIdxF] already set (:346)
                if (idx2 < nleft2) {
                    if (d < bestDist1) { bestDist2 = bestDist1; bestDist1 = d; bestIdxF = idx2; }
                    else if (d < bestDist2) bestDist2 = d;
                } else {
                    if (d < bestDist1R) { bestDist2R = bestDist1R; bestDist1R = d; bestIdxFR = idx2; }
                    else if (d < bestDist2R) bestDist2R = d;
                }
            }
            if (bestDist1 <= TH_LOW) {
                if (static_cast<float>(bestDist1) < nnratio * static_cast<float>(bestDist2)) {
                    assigned2[bestIdxF] = it.idx1;
                    nmatches++;
                    if (check_ori) hist.add(K1->keys_un[it.idx1].angle, K2->keys_un[bestIdxF].angle, bestIdxF);
                }
                if (bestDist1R <= TH_LOW) {
                    assigned2[bestIdxFR] = it.idx1;
                    nmatches++;
                    if (check_ori) hist.add(K1->keys_un[it.idx1].angle, K2->keys_un[bestIdxFR].angle, bestIdxFR);
                }
            }
        }
        if (check_ori) hist.prune([&](int idx2) { assigned2[idx2] = -1; nmatches--; });
    }
    if (nmatches_out) *nmatches_out = nmatches;
    return ORBX_OK;
}

// ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:734-880)
int orbm_search_for_initialization(orbx_extractor* h, const OrbmFrameView* F1, const OrbmFrameView* F2, float* prev, int window_size,
                                   float nnratio, int check_ori, int* matches12, int* nmatches_out) {
    if (!h || !F1 || !F2 || !prev || !matches12) return fail(ORBX_E_ARG, "null");
    rt::set_device(h->device);
    DeviceFrame D;
    int rc = upload_frame(h, F2, &D); if (rc) return rc;
    const int N1 = F1->N, N2 = F2->N;
    std::vector<AreaQuery> qs(N1);
    for (int i = 0; i < N1; i++) {
        AreaQuery& q = qs[i]; memset(&q, 0, sizeof q);
        const int level1 = F1->keys_un[i].octave;
        if (level1 > 0) continue;                                   // :755-757 only level-0 keypoints
        q.x = prev[2 * i]; q.y = prev[2 * i + 1]; q.r = (float)window_size; q.min_level = level1; q.max_level = level1; q.active = 1; q.gate = 0;
    }
    Cands c;
    rc = run_area_search(h, D, qs, F1->desc, &c); if (rc) return rc;
    for (int i = 0; i < N1; i++) matches12[i] = -1;
    std::vector<int> matched_dist(N2 > 0 ? N2 : 1, 0x7FFFFFFF), matches21(N2 > 0 ? N2 : 1, -1);
    RotHist hist;
    int nmatches = 0;
    for (int i1 = 0; i1 < N1; i1++) {
        if (!qs[i1].active || c.count[i1] == 0) continue;
        int bestDist = 0x7FFFFFFF, bestDist2 = 0x7FFFFFFF, bestIdx2 = -1;
        for (int k = 0; k < c.count[i1]; k++) {
            const int i2 = c.idx(i1, k), dist = c.dist(i1, k);
            if (matched_dist[i2] <= dist) continue;                    // :790 (not the occupancy skip of the other scans)
            if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestIdx2 = i2; }
            else if (dist < bestDist2) bestDist2 = dist;
        }
        if (bestDist <= TH_LOW) {
            if (bestDist < (float)bestDist2 * nnratio) {
                if (matches21[bestIdx2] >= 0) { matches12[matches21[bestIdx2]] = -1; nmatches--; }
                matches12[i1] = bestIdx2; matches21[bestIdx2] = i1; matched_dist[bestIdx2] = bestDist;
                nmatches++;
                if (check_ori) hist.add(F1->keys_un[i1].angle, F2->keys_un[bestIdx2].angle, i1);
            }
        }
    }
    if (check_ori) hist.prune([&](int idx1) { if (matches12[idx1] >= 0) { matches12[idx1] = -1; nmatches--; } });
    for (int i1 = 0; i1 < N1; i1++) if (matches12[i1] >= 0) { prev[2 * i1] = F2->keys_un[matches12[i1]].x; prev[2 * i1 + 1] = F2->keys_un[matches12[i1]].y; }
    if (nmatches_out) *nmatches_out = nmatches;
    return ORBX_OK;
}

}  // extern "C"

// ---- the remaining projection-type searches.  The caller evaluates the geometry (Sophus/Eigen op order
// stays the reference's) and hands over, per map point: valid (= survived every skip test in front of GetFeaturesInArea), the
// projection, the predicted level and the descriptor.  GetFeaturesInArea, the level window, the chi-square gate and all Hamming
// distances run on the GPU (k_area_search); the accept logic is replayed here over the ordered candidate lists.
namespace {

// one k_area_search over P's valid points: window radius th * scale[pred], levels [pred-1, pred+hi]
int projected_candidates(orbx_extractor* h, const OrbmFrameView* F, const OrbmProjectedPointView* P, float th, int hi, int gate,
                         const float* inv_sigma2, std::vector<AreaQuery>* qs, Cands* c) {
    if (!P || P->M < 0 || (P->M > 0 && (!P->valid || !P->u || !P->v || !P->pred_level || !P->desc))) return fail(ORBX_E_ARG, "bad point view");
    if (F && F->nlevels > kMaxLevels) return fail(ORBX_E_ARG, "too many levels");
    DeviceFrame D;
    int rc = upload_frame(h, F, &D); if (rc) return rc;
    if (gate == 2) {
        if (!inv_sigma2) return fail(ORBX_E_ARG, "chi-square gate without mvInvLevelSigma2");
        for (int l = 0; l < F->nlevels; l++) D.g.inv_sigma2[l] = inv_sigma2[l];
    }
    const int M = P->M;
    qs->resize(M);
    for (int i = 0; i < M; i++) {
        AreaQuery& q = (*qs)[i]; memset(&q, 0, sizeof q);
        if (!P->valid[i]) continue;
        const int lvl = P->pred_level[i];
        if (lvl < 0 || lvl >= F->nlevels) continue;
        q.x = P->u[i]; q.y = P->v[i]; q.r = th * F->scale_factors[lvl];
        q.ur = P->ur ? P->ur[i] : 0.0f;
        q.min_level = lvl - 1; q.max_level = lvl + hi; q.active = 1; q.gate = gate;
    }
    return run_area_search(h, D, *qs, P->desc, c);
}

}  // namespace

extern "C" {

int orbm_project_points(orbx_extractor* h, const OrbmProjection* S, const OrbmProjectIn* in, const OrbmProjectOut* out) {
    if (!h || !S || !in || !out || in->M < 0) return fail(ORBX_E_ARG, "null");
    const int M = in->M;
    if (M == 0) return ORBX_OK;
    if (!in->pos || (S->angle_test && !in->normal) || (S->distance_test && (!in->min_inv || !in->max_inv))) return fail(ORBX_E_ARG, "projection inputs missing");
    static_assert(sizeof(ProjectParams) == sizeof(OrbmProjection), "OrbmProjection and ProjectParams describe the same record");
    rt::set_device(h->device);
    const size_t M1 = M;
    const size_t op = 0, on = op + al16(12 * M1), omn = on + al16(12 * M1), omx = omn + al16(4 * M1), os = omx + al16(4 * M1), in_total = os + al16(M1);
    const size_t ov = 0, oo = al16(M1), out_total = oo + al16(20 * M1);
    if (h->h_packB.ensure(in_total + 16) || h->d_sr[SR_QUERY].ensure(in_total + 16) || h->d_sr[SR_SPARE].ensure(out_total + 16) || h->h_out.ensure(out_total + 16))
        return fail(ORBX_E_DEVICE, "allocation failed");
    uint8_t* hp = h->h_packB.p;
    memcpy(hp + op, in->pos, 12 * M1);
    if (in->normal) memcpy(hp + on, in->normal, 12 * M1);
    if (in->min_inv) memcpy(hp + omn, in->min_inv, 4 * M1);
    if (in->max_inv) memcpy(hp + omx, in->max_inv, 4 * M1);
    if (in->skip) memcpy(hp + os, in->skip, M1); else memset(hp + os, 0, M1);
    if (rt::copy_h2d(h->d_sr[SR_QUERY].p, hp, in_total, h->s0)) return fail(ORBX_E_DEVICE, "upload failed");
    ProjectParams P; memcpy(&P, S, sizeof P);
    const uint8_t* di = h->d_sr[SR_QUERY].p; uint8_t* dout = h->d_sr[SR_SPARE].p;
    dim3 grid((M + 255) / 256, 1, 1), blk(256, 1, 1);
    ORBX_LAUNCH(k_project_points, grid, blk, 0, h->s0, P, M, (const float*)(di + op), (const float*)(di + on), (const float*)(di + omn), (const float*)(di + omx),
                (const uint8_t*)(di + os), dout + ov, (float*)(dout + oo), h->debug_stereo_flags);
    if (rt::copy_d2h(h->h_out.p, dout, out_total, h->s0) || rt::stream_sync(h->s0) || rt::check_launch()) return fail(ORBX_E_DEVICE, "projection kernel failed: %s", rt::last_error());
    const float* f = (const float*)(h->h_out.p + oo);
    if (out->valid) memcpy(out->valid, h->h_out.p + ov, M1);
    if (out->u) memcpy(out->u, f, 4 * M1);
    if (out->v) memcpy(out->v, f + M1, 4 * M1);
    if (out->ur) memcpy(out->ur, f + 2 * M1, 4 * M1);
    if (out->inv_z) memcpy(out->inv_z, f + 3 * M1, 4 * M1);
    if (out->dist) memcpy(out->dist, f + 4 * M1, 4 * M1);
    return ORBX_OK;
}

int orbm_search_by_projection_sim3(orbx_extractor* h, const OrbmFrameView* KF, const OrbmProjectedPointView* P, float th, float ratio_hamming,
                                   int* assigned, int* nmatches_out) {
    if (!h || !KF || !P || !assigned) return fail(ORBX_E_ARG, "null");
    rt::set_device(h->device);
    std::vector<AreaQuery> qs; Cands c;
    int rc = projected_candidates(h, KF, P, th, 0, 0, nullptr, &qs, &c); if (rc) return rc;
    const int N = KF->N;
    std::vector<uint8_t> occ(N > 0 ? N : 1, 0);
    if (KF->occupied) memcpy(occ.data(), KF->occupied, N);          // vpMatched[idx] != NULL
    for (int i = 0; i < N; i++) assigned[i] = -1;
    int nmatches = 0;
    for (int i = 0; i < P->M; i++) {                                 // src/ORBmatcher.cc:519-606 / :640-727
        if (!qs[i].active || c.count[i] == 0) continue;
        const Best b = scan_best(c, i, occ.data());
        if (b.idx >= 0 && b.dist <= TH_LOW * ratio_hamming) { assigned[b.idx] = i; occ[b.idx] = 1; nmatches++; }
    }
    if (nmatches_out) *nmatches_out = nmatches;
    return ORBX_OK;
}

int orbm_search_by_projection_keyframe(orbx_extractor* h, const OrbmFrameView* Cur, const OrbmProjectedPointView* P, float th, int orb_dist,
                                       int check_ori, int* assigned, int* nmatches_out) {
    if (!h || !Cur || !P || !assigned) return fail(ORBX_E_ARG, "null");
    if (check_ori && P->M > 0 && !P->angle) return fail(ORBX_E_ARG, "orientation check without key-frame angles");
    rt::set_device(h->device);
    std::vector<AreaQuery> qs; Cands c;
    int rc = projected_candidates(h, Cur, P, th, 1, 0, nullptr, &qs, &c); if (rc) return rc;
    const int N = Cur->N;
    std::vector<uint8_t> occ(N > 0 ? N : 1, 0);
    if (Cur->occupied) memcpy(occ.data(), Cur->occupied, N);        // CurrentFrame.mvpMapPoints[i2] != NULL
    for (int i = 0; i < N; i++) assigned[i] = -1;
    RotHist hist;
    int nmatches = 0;
    for (int i = 0; i < P->M; i++) {                                 // src/ORBmatcher.cc:2213-2290
        if (!qs[i].active || c.count[i] == 0) continue;
        const Best b = scan_best(c, i, occ.data());
        if (b.idx >= 0 && b.dist <= orb_dist) {
            assigned[b.idx] = i; occ[b.idx] = 1; nmatches++;
            if (check_ori) hist.add(P->angle[i], Cur->keys_un[b.idx].angle, b.idx);
        }
    }
    if (check_ori) hist.prune([&](int idx) { assigned[idx] = -2; nmatches--; });
    if (nmatches_out) *nmatches_out = nmatches;
    return ORBX_OK;
}

int orbm_fuse_candidates(orbx_extractor* h, const OrbmFrameView* KF, const OrbmProjectedPointView* P, float th, int chi2_gate,
                         const float* inv_level_sigma2, int* best_idx, int* best_dist) {
    if (!h || !KF || !P || !best_idx) return fail(ORBX_E_ARG, "null");
    if (chi2_gate && P->M > 0 && !P->ur) return fail(ORBX_E_ARG, "chi-square gate without projected right coordinates");
    rt::set_device(h->device);
    std::vector<AreaQuery> qs; Cands c;
    int rc = projected_candidates(h, KF, P, th, 0, chi2_gate ? 2 : 0, inv_level_sigma2, &qs, &c); if (rc) return rc;
    for (int i = 0; i < P->M; i++) {                                 // src/ORBmatcher.cc:1421-1490 / :1601-1640
        const Best b = scan_best(c, i, nullptr);                     // no occupancy here; an inactive query has no candidates
        const int bestIdx = b.dist > TH_LOW ? -1 : b.idx;            // :1493 / :1643
        best_idx[i] = bestIdx;
        if (best_dist) best_dist[i] = bestIdx >= 0 ? b.dist : -1;
    }
    return ORBX_OK;
}

// Fuse's candidate search for one resident point set against K resident key frames.  One upload (the records of the grids to build, the target table, the
// skip mask), at most two launches (k_grid_build_kfs for the key frames that have no grid for their target's bounds yet, k_fuse_candidates), one download.
namespace {
const int kKfGridsKept = 2;             // grids a key frame keeps between calls (a key frame is normally searched with one set of bounds)
// the grids one call reads: found or made under the mutex, released when the call ends - whichever way
struct KfGridUse {
    std::vector<KfGrid*> held; std::vector<orbm_keyframe*> of;
    ~KfGridUse() {
        if (held.empty()) return;
        std::lock_guard<std::mutex> lk(kf_grid_mutex());
        for (KfGrid* g : held) g->users--;
        // kf_grid_for drops nothing that another call is reading, so beside other threads a list grows past kKfGridsKept: back to that, oldest first
        for (orbm_keyframe* kf : of)
            for (size_t i = 0; i < kf->grids.size() && (int)kf->grids.size() > kKfGridsKept;) {
                KfGrid* g = kf->grids[i];
                if (g->users == 0) { rt::dfree(g->mem); delete g; kf->grids.erase(kf->grids.begin() + i); } else i++;
            }
    }
};
// (caller holds the mutex) the grid of kf for `key`; *fresh = it has just been allocated and is still to be built
KfGrid* kf_grid_for(orbm_keyframe* kf, const float key[4], bool* fresh) {
    *fresh = false;
    // (an entry in use that is not built yet was made for an earlier target of THIS call: nobody else gets in while a call that builds holds the mutex)
    for (KfGrid* g : kf->grids) if ((g->built || g->users > 0) && !memcmp(g->key, key, sizeof g->key)) return g;
    const bool full = (int)kf->grids.size() >= kKfGridsKept;        // other bounds than before: drop what no call is reading
    for (size_t i = 0; i < kf->grids.size();) {
        KfGrid* g = kf->grids[i];
        if (g->users == 0 && (full || !g->built)) { rt::dfree(g->mem); delete g; kf->grids.erase(kf->grids.begin() + i); } else i++;
    }
    int* mem = (int*)rt::dmalloc(sizeof(int) * ((size_t)kGridCellStride + 2 * ((size_t)kf->N + 1)));
    if (!mem) return nullptr;
    KfGrid* g = new KfGrid();
    memcpy(g->key, key, sizeof g->key); g->mem = mem; g->users = 0; g->built = false;
    kf->grids.push_back(g);
    *fresh = true;
    return g;
}
// what orbm_fuse_candidates_batch and orbm_search_by_projection_sim3_batch refuse of target k alike
int batch_target_check(const orbx_extractor* h, int k, const orbm_keyframe* kf, const OrbmProjection& spec) {
    if (!kf) return fail(ORBX_E_ARG, "target %d: null key frame", k);
    if (kf->device != h->device) return fail(ORBX_E_ARG, "target %d: its key frame lives on another device than the handle", k);
    if (kf->nlevels < 1) return fail(ORBX_E_ARG, "target %d: its key frame has no scale levels", k);
    if (!(spec.max_x > spec.min_x) || !(spec.max_y > spec.min_y)) return fail(ORBX_E_ARG, "target %d: empty image bounds", k);
    return ORBX_OK;
}
// the grids the targets of one call read, found in the key frames' caches or made (`build`: the records k_grid_build_kfs takes for those).  Used under the mutex.
struct BatchGrids {
    KfGridUse use; std::vector<GridBuildRec> build; std::vector<KfGrid*> made;
    // (caller holds the mutex) fills R for one target: the key frame's arrays, the projection, the grid for the spec's bounds; false = the grid's allocation failed
    bool target(orbm_keyframe* kf, const OrbmProjection& spec, float log_scale_factor, const float* inv_level_sigma2, FuseTargetRec& R) {
        memset(&R, 0, sizeof R);
        memcpy(&R.P, &spec, sizeof R.P);
        R.g.min_x = spec.min_x; R.g.min_y = spec.min_y;
        R.g.gw_inv = (float)kGridColsHost / (spec.max_x - spec.min_x); R.g.gh_inv = (float)kGridRowsHost / (spec.max_y - spec.min_y);      // src/Frame.cc:190-191
        if (inv_level_sigma2) for (int l = 0; l < kf->nlevels; l++) R.g.inv_sigma2[l] = inv_level_sigma2[l];
        R.kps = kf->dev.kps; R.desc = kf->dev.desc; R.ur = kf->dev.ur;
        R.N = kf->N; R.nlevels = kf->nlevels; R.log_scale_factor = log_scale_factor;
        for (int l = 0; l < kMaxLevels; l++) R.scale_factors[l] = kf->scale[l];
        const float key[4] = {R.g.min_x, R.g.min_y, R.g.gw_inv, R.g.gh_inv};
        bool fresh;
        KfGrid* G = kf_grid_for(kf, key, &fresh);
        if (!G) return false;
        G->users++; use.held.push_back(G); use.of.push_back(kf);
        R.cell_start = G->mem; R.cell_items = G->mem + kGridCellStride;
        if (fresh) { GridBuildRec b; b.kps = kf->dev.kps; b.cell_of = G->mem + kGridCellStride + kf->N + 1; b.cell_start = G->mem; b.cell_items = G->mem + kGridCellStride; b.N = kf->N; b.g = R.g; build.push_back(b); made.push_back(G); }
        return true;
    }
    void launch_builds(orbx_extractor* h, const GridBuildRec* dev) const {
        if (build.empty()) return;
        const dim3 gridb((unsigned)build.size(), 1, 1), blkb(kGridThreads, 1, 1);
        ORBX_LAUNCH(k_grid_build_kfs, gridb, blkb, 0, h->s0, dev);
    }
    void built() { for (KfGrid* g : made) g->built = true; }         // (the stream has been waited for; still under the mutex: `made` is empty otherwise)
};

// What a call that is fed from the map (orbm_fuse_candidates_batch_map, orbm_search_by_projection_sim3_batch_map, at the end of this file) brings in place
// of the host's skip[K][M]: the set's slot list, the slots' states and the map's rows on the device, one MapSkipRec per target, and - Sim3 - the found lists
// to upload.  The entry point has checked everything and holds the map's mutex until the call returns; map_skip_table() gives the call its range of the
// map's table by slot (allocated on the first such call) once nothing can be refused any more.
struct MapSkip {
    orbm_map* map; const int* set_slots; const uint8_t* state; const int* kf_slots;
    std::vector<MapSkipRec> recs; int longest = 0;
    const int* found = nullptr; size_t n_found = 0;                 // host: the found lists, one behind the other (nullptr: the lists are the map's rows)
    unsigned* table = nullptr; unsigned base = 0, top = 0;
};
int map_skip_table(orbx_extractor* h, int M, MapSkip* S);
// skip[K][M] on the device (k_search.hip "the exclusions of a Fuse / Sim3 projection batch read from the map")
void launch_map_skip(orbx_extractor* h, const MapSkip& S, int K, int M, const MapSkipRec* d_recs, const int* d_lists, uint8_t* d_skip) {
    const dim3 blk(256, 1, 1), grids((M + 255) / 256, (K + kSkipTargets - 1) / kSkipTargets, 1);
    ORBX_LAUNCH(k_map_set_table, grids, blk, 0, h->s0, M, K, S.set_slots, S.state, S.table, S.top, d_skip);
    if (S.longest > 0) {
        const dim3 gridl((S.longest + 255) / 256, K, 1);
        ORBX_LAUNCH(k_map_skip_listed, gridl, blk, 0, h->s0, d_recs, d_lists, M, (const unsigned*)S.table, S.base, S.top, d_skip);
        ORBX_LAUNCH(k_map_skip_dups, grids, blk, 0, h->s0, M, K, S.set_slots, (const unsigned*)S.table, S.top, d_skip);
    }
}

// what orbm_fuse_candidates_batch and its map-fed form refuse of the target table alike
int fuse_targets_check(const orbx_extractor* h, int K, const OrbmFuseTarget* targets, int chi2_gate) {
    if (!targets) return fail(ORBX_E_ARG, "null target table");
    static_assert(sizeof(ProjectParams) == sizeof(OrbmProjection), "OrbmProjection and ProjectParams describe the same record");
    for (int k = 0; k < K; k++) {
        const OrbmFuseTarget& t = targets[k];
        if (int rc = batch_target_check(h, k, t.kf, t.spec)) return rc;
        if (chi2_gate && !t.inv_level_sigma2) return fail(ORBX_E_ARG, "target %d: chi-square gate without mvInvLevelSigma2", k);
    }
    return ORBX_OK;
}

// The compacted form of the Fuse batch's answer (orbm_fuse_pairs_batch / orbm_fuse_pairs_batch_map): the caller's arrays, and where everything lies in the
// handle's d_si[SI_BEST], in ints: the dense best_idx [and best_dist] of the search, the chunk counts and offsets, the tile sums and offsets
// (k_search.hip "the matched pairs of a Fuse batch as one list"), and - one behind the other, so that one copy brings both - start[K + 1] and the records
struct FusePairsWanted { int cap; int* start; int* point; int* feat; int* dist; int* point_slot; int* kf_slot; };
struct FusePairsLayout {
    size_t nch = 0, ntiles = 0, dcap = 0, o_cnt = 0, o_off = 0, o_tsum = 0, o_toff = 0, o_start = 0, o_rec = 0, ints = 0;
    int fields = 0, f_dist = -1, f_pslot = -1, f_kfs = -1;
    FusePairsLayout() {}
    FusePairsLayout(const FusePairsWanted& W, int K, int M) {
        const size_t pairs = (size_t)K * (size_t)M;
        nch = (size_t)K * (size_t)((M + kPairChunk - 1) / kPairChunk); ntiles = (nch + kPairTile - 1) / kPairTile;
        dcap = std::min((size_t)W.cap, pairs);                      // (a list longer than cap is not written)
        fields = 2;
        if (W.dist) f_dist = fields++;
        if (W.point_slot) f_pslot = fields++;
        if (W.kf_slot) f_kfs = fields++;
        o_cnt = (W.dist ? 2 : 1) * pairs; o_off = o_cnt + nch; o_tsum = o_off + nch; o_toff = o_tsum + ntiles; o_start = o_toff + ntiles + 1;
        o_rec = o_start + (size_t)K + 1; ints = o_rec + dcap * (size_t)fields;
    }
};
// records [r0, r1) of the list, as they came down, into the caller's arrays
void fuse_pairs_unpack(const FusePairsWanted& W, const FusePairsLayout& L, const int* rec, size_t r0, size_t r1) {
    for (size_t r = r0; r < r1; r++, rec += L.fields) {
        W.point[r] = rec[0]; W.feat[r] = rec[1];
        if (W.dist) W.dist[r] = rec[L.f_dist];
        if (W.point_slot) W.point_slot[r] = rec[L.f_pslot];
        if (W.kf_slot) W.kf_slot[r] = rec[L.f_kfs];
    }
}
// Behind k_fuse_candidates on the same stream: count, scan, scatter, and the download.  `start` comes down first and with it, in the same copy, the first
// `guess` records - a quarter more than the handle's last such call found, at least 1024: a call whose list is that short (LocalMapping's, and every
// repeat of a call at a steady scene) waits for the stream once, where a second wait costs more than the few KB that may not be needed; only a longer list
// pays a second copy, of exactly the records that are missing.
int fuse_pairs_finish(orbx_extractor* h, int K, int M, const FusePairsWanted& W, const FusePairsLayout& L, const MapSkip* from_map, const MapSkipRec* d_recs,
                      BatchGrids& grids) {
    int* d = h->d_si[SI_BEST].p;
    const size_t pairs = (size_t)K * (size_t)M;
    const dim3 grid((M + kPairChunk - 1) / kPairChunk, K, 1), blk(kPairChunk, 1, 1), gridt((unsigned)((L.nch + 255) / 256), 1, 1), blkt(256, 1, 1), one(1, 1, 1);
    const FusePairOut O = {d + L.o_rec, L.fields, L.f_dist, L.f_pslot, L.f_kfs};
    const int* d_dist = W.dist ? d + pairs : (const int*)nullptr;
    const int* kf_slots = from_map ? from_map->kf_slots : (const int*)nullptr; const uint8_t* state = from_map ? from_map->state : (const uint8_t*)nullptr;
    const int* set_slots = from_map ? from_map->set_slots : (const int*)nullptr;
    ORBX_LAUNCH(k_fuse_pairs, grid, blk, 0, h->s0, M, (const int*)d, d_dist, d + L.o_cnt, (const int*)nullptr, (const int*)nullptr, (int)L.ntiles, W.cap, d + L.o_start,
                d_recs, kf_slots, state, set_slots, O);
    ORBX_LAUNCH(k_fuse_pair_scan_tiles, gridt, blkt, 0, h->s0, (int)L.nch, (const int*)(d + L.o_cnt), d + L.o_off, d + L.o_tsum);
    ORBX_LAUNCH(k_fuse_pair_scan_sums, one, blkt, 0, h->s0, (int)L.ntiles, (const int*)(d + L.o_tsum), d + L.o_toff);
    ORBX_LAUNCH(k_fuse_pairs, grid, blk, 0, h->s0, M, (const int*)d, d_dist, d + L.o_cnt, (const int*)(d + L.o_off), (const int*)(d + L.o_toff), (int)L.ntiles, W.cap,
                d + L.o_start, d_recs, kf_slots, state, set_slots, O);
    const size_t guess = std::min(L.dcap, std::max<size_t>(h->fuse_pairs_last + h->fuse_pairs_last / 4 + 256, 1024)), head = (size_t)K + 1;
    const bool direct = rt::memory_is_host();
    const int* res = d + L.o_start;
    int e = 0;
    if (!direct) {
        e = h->h_res.ensure(sizeof(int) * (head + guess * L.fields) + 64);
        if (!e) e = rt::copy_d2h(h->h_res.p, d + L.o_start, sizeof(int) * (head + guess * L.fields), h->s0);
        res = (const int*)h->h_res.p;
    }
    if (e || rt::stream_sync(h->s0) || rt::check_launch()) return fail(ORBX_E_DEVICE, "fuse pair search failed: %s", rt::last_error());
    grids.built();
    memcpy(W.start, res, sizeof(int) * head);
    const size_t total = (size_t)W.start[K];
    if (total > (size_t)W.cap) return fail(ORBX_E_CAPACITY, "%zu pairs do not fit in cap = %d", total, W.cap);
    h->fuse_pairs_last = total;
    fuse_pairs_unpack(W, L, res + head, 0, std::min(total, guess));
    if (total > guess) {
        const int* rest = d + L.o_rec + guess * L.fields;
        if (!direct) {
            const size_t bytes = sizeof(int) * (total - guess) * L.fields;
            if (h->h_res.ensure(bytes + 64) || rt::copy_d2h(h->h_res.p, rest, bytes, h->s0) || rt::stream_sync(h->s0))
                return fail(ORBX_E_DEVICE, "fuse pair download failed: %s", rt::last_error());
            rest = (const int*)h->h_res.p;
        }
        fuse_pairs_unpack(W, L, rest, guess, total);
    }
    return ORBX_OK;
}

// The Fuse batch behind its checks, K > 0 checked targets: skip = the host's [K][M] bytes or nullptr; from_map: the bytes are written on the device where
// `skip` would have been uploaded, and kf_slot (may be nullptr) comes back behind the distances.  want: the pair-list forms - the dense result stays on the
// device and fuse_pairs_finish takes over behind the search (best_idx, best_dist and kf_slot are not read then)
int fuse_batch_run(orbx_extractor* h, int K, const OrbmFuseTarget* targets, const orbm_points* points, const uint8_t* skip, MapSkip* from_map, float th, int chi2_gate,
                   int* best_idx, int* best_dist, int* kf_slot, const FusePairsWanted* want = nullptr) {
    const int M = points->M;
    if (M == 0) { if (want) std::fill(want->start, want->start + K + 1, 0); return ORBX_OK; }
    if (!want && !best_idx) return fail(ORBX_E_ARG, "null result array");
    if (K > 65535 || (size_t)K * (size_t)M > ((size_t)1 << 28)) return fail(ORBX_E_CAPACITY, "%d targets x %d points: at most 65535 targets and 2^28 pairs per call", K, M);
    rt::set_device(h->device);
    const size_t pairs = (size_t)K * (size_t)M;
    std::vector<FuseTargetRec> recs(K);
    BatchGrids grids;
    std::unique_lock<std::mutex> lk(kf_grid_mutex());
    for (int k = 0; k < K; k++) {
        const OrbmFuseTarget& t = targets[k];
        // (the grid cache is the one part of a resident key frame that a search adds to)
        if (!grids.target(const_cast<orbm_keyframe*>(t.kf), t.spec, t.log_scale_factor, chi2_gate ? t.inv_level_sigma2 : nullptr, recs[k]))
            return fail(ORBX_E_DEVICE, "target %d: allocation of its grid failed", k);
    }
    // a grid made here is built on this handle's stream: other threads may find it in the list, so they are kept out until this call has waited for the stream
    if (grids.build.empty()) lk.unlock();
    Packer pk(h);
    const size_t pb = pk.add(grids.build.data(), sizeof(GridBuildRec) * grids.build.size()), pt = pk.add(recs.data(), sizeof(FuseTargetRec) * recs.size());
    const size_t pr = from_map ? pk.add(from_map->recs.data(), sizeof(MapSkipRec) * from_map->recs.size()) : 0;
    const size_t ps = from_map ? pk.room(pairs) : skip ? pk.add(skip, pairs) : 0;
    const bool flags = from_map || skip;
    const FusePairsLayout PL = want ? FusePairsLayout(*want, K, M) : FusePairsLayout();
    const size_t nout = want ? PL.ints : (1 + (best_dist ? 1 : 0) + (kf_slot ? 1 : 0)) * pairs;
    if (h->d_si[SI_BEST].ensure(nout)) return fail(ORBX_E_DEVICE, "allocation failed (%d targets x %d points)", K, M);
    if (from_map) if (int rc = map_skip_table(h, M, from_map)) return rc;
    if (int e = pk.flush()) return fail(ORBX_E_DEVICE, "%s", upload_error(e));
    grids.launch_builds(h, pk.dev<GridBuildRec>(pb));
    if (from_map) launch_map_skip(h, *from_map, K, M, pk.dev<MapSkipRec>(pr), from_map->kf_slots, pk.out<uint8_t>(ps));
    int* d_idx = h->d_si[SI_BEST].p; int* d_dist = (want ? want->dist : best_dist) ? d_idx + pairs : (int*)nullptr; int* d_kfs = d_idx + (best_dist ? 2 : 1) * pairs;
    const dim3 grid((M + 255) / 256, K, 1), blk(256, 1, 1);
    ORBX_LAUNCH(k_fuse_candidates, grid, blk, 0, h->s0, pk.dev<FuseTargetRec>(pt), M, points->pos, points->normal, points->min_d, points->max_d, points->desc,
                flags ? pk.dev<uint8_t>(ps) : (const uint8_t*)nullptr, th, chi2_gate, TH_LOW, h->debug_stereo_flags, d_idx, d_dist);
    if (want) return fuse_pairs_finish(h, K, M, *want, PL, from_map, from_map ? pk.dev<MapSkipRec>(pr) : (const MapSkipRec*)nullptr, grids);
    if (kf_slot) ORBX_LAUNCH(k_fuse_kf_slots, grid, blk, 0, h->s0, pk.dev<MapSkipRec>(pr), from_map->kf_slots, M, from_map->state, (const int*)d_idx, d_kfs);
    // one copy into the handle's page-locked landing area (as fetch_sync), then into the caller's one to three arrays
    const int* res = d_idx;
    int e = 0;
    if (!rt::memory_is_host()) {
        e = h->h_res.ensure(sizeof(int) * nout + 64);
        if (!e) e = rt::copy_d2h(h->h_res.p, d_idx, sizeof(int) * nout, h->s0);
        res = (const int*)h->h_res.p;
    }
    if (e || rt::stream_sync(h->s0) || rt::check_launch()) return fail(ORBX_E_DEVICE, "fuse candidate search failed: %s", rt::last_error());
    grids.built();
    memcpy(best_idx, res, sizeof(int) * pairs);
    if (best_dist) memcpy(best_dist, res + pairs, sizeof(int) * pairs);
    if (kf_slot) memcpy(kf_slot, res + (best_dist ? 2 : 1) * pairs, sizeof(int) * pairs);
    return ORBX_OK;
}

// what the pair-list forms refuse of their own arguments
int fuse_pairs_check(int cap, const int* start, const int* point, const int* feat) {
    if (cap < 0) return fail(ORBX_E_ARG, "negative cap");
    if (!start) return fail(ORBX_E_ARG, "null start array");
    if (cap > 0 && (!point || !feat)) return fail(ORBX_E_ARG, "null point or feat array with cap = %d", cap);
    return ORBX_OK;
}

// what orbm_search_by_projection_sim3_batch and its map-fed form refuse of the target table alike; *n_max = the largest N
int sim3_targets_check(const orbx_extractor* h, int K, const OrbmSim3Target* targets, int cap, int* n_max) {
    if (!targets) return fail(ORBX_E_ARG, "null target table");
    *n_max = 0;
    for (int k = 0; k < K; k++) {
        if (int rc = batch_target_check(h, k, targets[k].kf, targets[k].spec)) return rc;
        *n_max = std::max(*n_max, targets[k].kf->N);
    }
    if (cap < *n_max) return fail(ORBX_E_ARG, "cap %d is below the %d keypoints of the largest key frame", cap, *n_max);
    return ORBX_OK;
}

// The Sim3 projection search of one resident point set from K resident key frames, behind its checks.  One upload (the records of the grids to build, the
// target table, the `occupied` rows, the skip mask - from_map: the MapSkipRec table and the found lists in its place), at most three launches
// (k_grid_build_kfs, k_sim3_candidates, k_sim3_accept; from_map: the three flag kernels in front, k_assigned_slots behind when assigned_slot is wanted), one
// download of assigned | nmatches [| assigned_slot].
int sim3_batch_run(orbx_extractor* h, int K, const OrbmSim3Target* targets, int n_max, const orbm_points* points, const uint8_t* skip, MapSkip* from_map, float th,
                   float ratio_hamming, int cap, int* assigned, int* nmatches, int* assigned_slot) {
    const int M = points->M;
    if (M == 0) return ORBX_OK;
    if (!assigned || !nmatches) return fail(ORBX_E_ARG, "null result array");
    const size_t lim = (size_t)1 << 28, cap1 = (size_t)std::max(cap, 1);
    if (K > 65535 || (size_t)K * (size_t)M > lim || (size_t)K * cap1 > lim)
        return fail(ORBX_E_CAPACITY, "%d targets x %d points (cap %d): at most 65535 targets, 2^28 pairs and 2^28 result entries per call", K, M, cap);
    rt::set_device(h->device);
    const size_t pairs = (size_t)K * (size_t)M, nres = (size_t)K * cap1 + (size_t)K + (assigned_slot ? (size_t)K * cap1 : 0);
    std::vector<Sim3TargetRec> recs(K);
    std::vector<uint8_t> occ;
    BatchGrids grids;
    std::unique_lock<std::mutex> lk(kf_grid_mutex());
    for (int k = 0; k < K; k++) {
        const OrbmSim3Target& t = targets[k];
        if (!grids.target(const_cast<orbm_keyframe*>(t.kf), t.spec, t.log_scale_factor, nullptr, recs[k].F))
            return fail(ORBX_E_DEVICE, "target %d: allocation of its grid failed", k);
        recs[k].occ_off = -1;
        if (t.occupied && t.kf->N > 0) { recs[k].occ_off = (long long)occ.size(); occ.insert(occ.end(), t.occupied, t.occupied + t.kf->N); occ.resize(al16(occ.size()), 0); }
    }
    if (grids.build.empty()) lk.unlock();                            // (as in fuse_batch_run)
    Packer pk(h);
    const size_t pb = pk.add(grids.build.data(), sizeof(GridBuildRec) * grids.build.size()), pt = pk.add(recs.data(), sizeof(Sim3TargetRec) * recs.size()),
                 po = pk.add(occ.data(), occ.size());
    size_t pr = 0, pf = 0, pa = 0, ps = 0;
    std::vector<SetFlagRec> set_recs;
    if (from_map) {
        pr = pk.add(from_map->recs.data(), sizeof(MapSkipRec) * from_map->recs.size());
        pf = pk.add(from_map->found, sizeof(int) * from_map->n_found);
        if (assigned_slot) { set_recs.assign(K, SetFlagRec{nullptr, from_map->set_slots, M, 0}); pa = pk.add(set_recs.data(), sizeof(SetFlagRec) * set_recs.size()); }
        ps = pk.room(pairs);
    } else if (skip) ps = pk.add(skip, pairs);
    const bool flags = from_map || skip;
    if (h->d_si[SI_BEST].ensure(pairs + nres)) return fail(ORBX_E_DEVICE, "allocation failed (%d targets x %d points, cap %d)", K, M, cap);
    if (from_map) if (int rc = map_skip_table(h, M, from_map)) return rc;
    if (int e = pk.flush()) return fail(ORBX_E_DEVICE, "%s", upload_error(e));
    grids.launch_builds(h, pk.dev<GridBuildRec>(pb));
    if (from_map) launch_map_skip(h, *from_map, K, M, pk.dev<MapSkipRec>(pr), pk.dev<int>(pf), pk.out<uint8_t>(ps));
    int* d_choice = h->d_si[SI_BEST].p; int* d_assigned = d_choice + pairs; int* d_nm = d_assigned + (size_t)K * cap1; int* d_aslot = d_nm + K;
    const Sim3TargetRec* d_tab = pk.dev<Sim3TargetRec>(pt);
    const float max_dist = (float)TH_LOW * ratio_hamming;            // `TH_LOW * ratioHamming` (:609 / :722): int * float
    const dim3 grid((M + 255) / 256, K, 1), blk(256, 1, 1), grida(K, 1, 1), blka(64, 1, 1);
    ORBX_LAUNCH(k_sim3_candidates, grid, blk, 0, h->s0, d_tab, M, points->pos, points->normal, points->min_d, points->max_d, points->desc, pk.dev<uint8_t>(po),
                flags ? pk.dev<uint8_t>(ps) : (const uint8_t*)nullptr, th, max_dist, h->debug_stereo_flags, d_choice);
    const size_t smem = al16(4 * (size_t)((n_max + 31) / 32)) + 16;
    ORBX_LAUNCH(k_sim3_accept, grida, blka, smem, h->s0, d_tab, M, points->pos, points->normal, points->min_d, points->max_d, points->desc, pk.dev<uint8_t>(po), th,
                max_dist, h->debug_stereo_flags, (int)cap1, (const int*)d_choice, d_assigned, d_nm);
    if (assigned_slot) {
        const dim3 grids((unsigned)((cap1 + 255) / 256), K, 1);
        ORBX_LAUNCH(k_assigned_slots, grids, blk, 0, h->s0, pk.dev<SetFlagRec>(pa), (const int*)d_assigned, (int)cap1, d_aslot);
    }
    const int* res = d_assigned;
    int e = 0;
    if (!rt::memory_is_host()) {
        e = h->h_res.ensure(sizeof(int) * nres + 64);
        if (!e) e = rt::copy_d2h(h->h_res.p, d_assigned, sizeof(int) * nres, h->s0);
        res = (const int*)h->h_res.p;
    }
    if (e || rt::stream_sync(h->s0) || rt::check_launch()) return fail(ORBX_E_DEVICE, "Sim3 projection search failed: %s", rt::last_error());
    grids.built();
    if (cap > 0) memcpy(assigned, res, sizeof(int) * (size_t)K * (size_t)cap);
    memcpy(nmatches, res + (size_t)K * cap1, sizeof(int) * (size_t)K);
    if (assigned_slot && cap > 0) memcpy(assigned_slot, res + (size_t)K * cap1 + (size_t)K, sizeof(int) * (size_t)K * (size_t)cap);
    return ORBX_OK;
}
}  // namespace

int orbm_fuse_candidates_batch(orbx_extractor* h, int K, const OrbmFuseTarget* targets, const orbm_points* points, const uint8_t* skip, float th, int chi2_gate,
                               int* best_idx, int* best_dist) {
    if (!h || !points || K < 0) return fail(ORBX_E_ARG, "null / negative number of targets");
    if (points->device != h->device) return fail(ORBX_E_ARG, "the map points live on another device than the handle");
    if (K == 0) return ORBX_OK;
    if (int rc = fuse_targets_check(h, K, targets, chi2_gate)) return rc;
    return fuse_batch_run(h, K, targets, points, skip, nullptr, th, chi2_gate, best_idx, best_dist, nullptr);
}

int orbm_fuse_pairs_batch(orbx_extractor* h, int K, const OrbmFuseTarget* targets, const orbm_points* points, const uint8_t* skip, float th, int chi2_gate, int cap,
                          int* start, int* point, int* feat, int* dist) {
    if (!h || !points || K < 0) return fail(ORBX_E_ARG, "null / negative number of targets");
    if (points->device != h->device) return fail(ORBX_E_ARG, "the map points live on another device than the handle");
    if (int rc = fuse_pairs_check(cap, start, point, feat)) return rc;
    if (K == 0) { start[0] = 0; return ORBX_OK; }
    if (int rc = fuse_targets_check(h, K, targets, chi2_gate)) return rc;
    const FusePairsWanted W = {cap, start, point, feat, dist, nullptr, nullptr};
    return fuse_batch_run(h, K, targets, points, skip, nullptr, th, chi2_gate, nullptr, nullptr, nullptr, &W);
}

int orbm_search_by_projection_sim3_batch(orbx_extractor* h, int K, const OrbmSim3Target* targets, const orbm_points* points, const uint8_t* skip, float th,
                                         float ratio_hamming, int cap, int* assigned, int* nmatches) {
    if (!h || !points || K < 0) return fail(ORBX_E_ARG, "null / negative number of targets");
    if (points->device != h->device) return fail(ORBX_E_ARG, "the map points live on another device than the handle");
    if (K == 0) return ORBX_OK;
    int n_max = 0;
    if (int rc = sim3_targets_check(h, K, targets, cap, &n_max)) return rc;
    return sim3_batch_run(h, K, targets, n_max, points, skip, nullptr, th, ratio_hamming, cap, assigned, nmatches, nullptr);
}

int orbm_search_by_sim3(orbx_extractor* h, const OrbmFrameView* KF1, const OrbmFrameView* KF2, const OrbmProjectedPointView* P1in2,
                        const OrbmProjectedPointView* P2in1, float th, int* matches12, int* nfound_out) {
    if (!h || !KF1 || !KF2 || !P1in2 || !P2in1 || !matches12) return fail(ORBX_E_ARG, "null");
    if (P1in2->M != KF1->N || P2in1->M != KF2->N) return fail(ORBX_E_ARG, "one projected point per key-frame feature expected");
    rt::set_device(h->device);
    const int N1 = KF1->N, N2 = KF2->N;
    std::vector<int> vnMatch1(N1 > 0 ? N1 : 1, -1), vnMatch2(N2 > 0 ? N2 : 1, -1);
    for (int dir = 0; dir < 2; dir++) {                              // src/ORBmatcher.cc:1735-1826 and :1829-1915
        const OrbmProjectedPointView* P = dir == 0 ? P1in2 : P2in1;
        std::vector<AreaQuery> qs; Cands c;
        int rc = projected_candidates(h, dir == 0 ? KF2 : KF1, P, th, 0, 0, nullptr, &qs, &c); if (rc) return rc;
        std::vector<int>& out = dir == 0 ? vnMatch1 : vnMatch2;
        for (int i = 0; i < P->M; i++) {
            if (!qs[i].active) continue;
            const Best b = scan_best(c, i, nullptr, 0, 0x7fffffff);
            if (b.dist <= TH_HIGH) out[i] = b.idx;
        }
    }
    int nfound = 0;
    for (int i1 = 0; i1 < N1; i1++) {                                // :1918-1932
        matches12[i1] = -1;
        const int idx2 = vnMatch1[i1];
        if (idx2 >= 0 && vnMatch2[idx2] == i1) { matches12[i1] = idx2; nfound++; }
    }
    if (nfound_out) *nfound_out = nfound;
    return ORBX_OK;
}

int orbm_distinctive_descriptors(orbx_extractor* h, const uint8_t* desc, const int* start, int P, int* best) {
    if (!h || P < 0 || (P > 0 && (!start || !best))) return fail(ORBX_E_ARG, "null");
    if (P == 0) return ORBX_OK;
    rt::set_device(h->device);
    const int total = start[P];
    if (total < 0 || (total > 0 && !desc)) return fail(ORBX_E_ARG, "bad descriptor list");
    for (int p = 0; p < P; p++) if (start[p + 1] < start[p]) return fail(ORBX_E_ARG, "start[] must be non-decreasing");
    int e = upload(h, SR_DESC, desc, 32 * (size_t)total) | h->d_si[SI_QSTART].ensure(P + 1) | h->d_si[SI_BEST].ensure(P);
    if (!e) e = rt::copy_h2d(h->d_si[SI_QSTART].p, start, sizeof(int) * (size_t)(P + 1), h->s0);
    if (e) return fail(ORBX_E_DEVICE, "upload/allocation failed");
    dim3 grid((P + 3) / 4, 1, 1), blk(256, 1, 1);
    ORBX_LAUNCH(k_distinctive, grid, blk, 0, h->s0, (const unsigned long long*)h->d_sr[SR_DESC].p, (const int*)h->d_si[SI_QSTART].p, P, h->d_si[SI_BEST].p);
    if (fetch_sync(h, best, h->d_si[SI_BEST].p, sizeof(int) * (size_t)P) || rt::check_launch()) return fail(ORBX_E_DEVICE, "distinctive-descriptor kernel failed: %s", rt::last_error());
    return ORBX_OK;
}

// ---- two-camera (Frame::Nleft != -1) branches.  Each camera's window search runs on the device (one k_area_search per camera); the
// reference interleaves the two cameras per map point and its assignments feed the occupancy test of later points, so the accept
// logic is replayed here over both candidate lists in the reference's order.
namespace {
int camera_candidates(orbx_extractor* h, const OrbmFrameView* F, const std::vector<AreaQuery>& qs, const uint8_t* qdesc, Csr* c) {
    DeviceFrame D;
    int rc = upload_frame(h, F, &D); if (rc) return rc;
    Cands v;
    rc = run_area_search(h, D, qs, qdesc, &v); if (rc) return rc;
    c->copy(v, (int)qs.size());
    return ORBX_OK;
}
}  // namespace

int orbm_search_by_projection_mappoints_fisheye(orbx_extractor* h, const OrbmFisheyeFrameView* F, const OrbmMapPointView* P,
                                                const OrbmMapPointRightView* PR, float th, int far_points, float th_far, float nnratio,
                                                int* assigned, int* nmatches_out) {
    if (!h || !F || !P || !PR || !assigned) return fail(ORBX_E_ARG, "null");
    rt::set_device(h->device);
    const int M = P->M, NL = F->left.N, NR = F->right.N;
    const bool bFactor = th != 1.0;
    std::vector<AreaQuery> ql(M), qr(M);
    std::vector<uint8_t> alive(M > 0 ? M : 1, 0);
    for (int i = 0; i < M; i++) {
        memset(&ql[i], 0, sizeof(AreaQuery)); memset(&qr[i], 0, sizeof(AreaQuery));
        const bool inl = P->in_view[i] != 0, inr = PR->in_view_r[i] != 0;
        if (!inl && !inr) continue;                                       // :53-60
        if (far_points && P->track_depth[i] > th_far) continue;
        if (P->is_bad[i]) continue;
        alive[i] = 1;
        if (inl) {
            const int lvl = P->scale_level[i];
            if (lvl >= 0 && lvl < F->left.nlevels) {
                float r = P->view_cos[i] > 0.998 ? 2.5f : 4.0f;
                if (bFactor) r *= th;
                AreaQuery& q = ql[i];
                q.x = P->proj_x[i]; q.y = P->proj_y[i]; q.r = r * F->left.scale_factors[lvl]; q.min_level = lvl - 1; q.max_level = lvl; q.active = 1;
            }
        }
        if (inr) {
            const int lvl = PR->scale_level_r[i];
            if (lvl != -1 && lvl >= 0 && lvl < F->right.nlevels) {            // :172-173
                const float r = PR->view_cos_r[i] > 0.998 ? 2.5f : 4.0f;     // the right pass does not apply th (:174)
                AreaQuery& q = qr[i];
                q.x = PR->proj_xr[i]; q.y = PR->proj_yr[i]; q.r = r * F->right.scale_factors[lvl]; q.min_level = lvl - 1; q.max_level = lvl; q.active = 1;
            }
        }
    }
    Csr csl, csr;
    int rc = camera_candidates(h, &F->left, ql, P->desc, &csl); if (rc) return rc;
    rc = camera_candidates(h, &F->right, qr, P->desc, &csr); if (rc) return rc;
    const Cands cl(csl), cr(csr);
    std::vector<uint8_t> occ((size_t)NL + NR + 1, 0);
    if (F->left.occupied) memcpy(occ.data(), F->left.occupied, NL);
    if (F->right.occupied) memcpy(occ.data() + NL, F->right.occupied, NR);
    for (int i = 0; i < NL + NR; i++) assigned[i] = -1;
    int nmatches = 0;
    for (int i = 0; i < M; i++) {
        if (!alive[i]) continue;
        const uint8_t obs = P->has_obs ? P->has_obs[i] : 1;
        bool skip_right = false;
        if (ql[i].active && cl.count[i] > 0) {                               // :62-166
            const Best2 b = scan_best2(cl, i, occ.data());
            if (b.bestDist <= TH_HIGH) {
                if (b.bestLevel == b.bestLevel2 && b.bestDist > nnratio * b.bestDist2) skip_right = true;     // `continue` of the reference: next map point
                else if (b.bestLevel != b.bestLevel2 || b.bestDist <= nnratio * b.bestDist2) {
                    assigned[b.bestIdx] = i; occ[b.bestIdx] = obs;
                    const int ltr = F->left_to_right ? F->left_to_right[b.bestIdx] : -1;
                    if (ltr != -1) { assigned[ltr + NL] = i; occ[ltr + NL] = obs; nmatches++; }
                    nmatches++;
                }
            }
        }
        if (skip_right) continue;
        if (qr[i].active) {                                                  // :170-236
            if (cr.count[i] == 0) continue;
            const Best2 b = scan_best2(cr, i, occ.data(), NL);
            if (b.bestDist <= TH_HIGH) {
                if (b.bestLevel == b.bestLevel2 && b.bestDist > nnratio * b.bestDist2) continue;
                const int rtl = F->right_to_left ? F->right_to_left[b.bestIdx] : -1;
                if (rtl != -1) { assigned[rtl] = i; occ[rtl] = obs; nmatches++; }
                assigned[b.bestIdx + NL] = i; occ[b.bestIdx + NL] = obs;
                nmatches++;
            }
        }
    }
    if (nmatches_out) *nmatches_out = nmatches;
    return ORBX_OK;
}

int orbm_search_local_points_fisheye(orbx_extractor* h, const OrbmFisheyeFrameView* F, const OrbmFrustumRigView* V, const OrbmWorldPointView* P, float cos_limit, float th,
                                     int far_points, float th_far, float nnratio, const OrbmTrackOut* left, const OrbmTrackOutRight* right, int* assigned, int* nmatches_out) {
    if (!h || !F || !V || !P || !assigned) return fail(ORBX_E_ARG, "null");
    if (P->M < 0 || (P->M > 0 && (!P->pos || !P->normal || !P->min_distance || !P->max_distance || !P->desc))) return fail(ORBX_E_ARG, "bad map point view");
    const size_t M1 = P->M > 0 ? P->M : 1;
    // the tracking fields of both cameras come back once (they are the reference's MapPoint members; the searches read them as views): into the
    // caller's arrays where they are given, into scratch where not
    std::vector<uint8_t> inl(M1), inr(M1), zero(M1, 0), one(M1, 1);
    std::vector<float> f(9 * M1);
    std::vector<int> ll(M1), lr(M1);
    const OrbmTrackOut l0 = left ? *left : OrbmTrackOut{};
    const OrbmTrackOutRight r0 = right ? *right : OrbmTrackOutRight{};
    const auto or_own = [](auto* given, auto* own) { return given ? given : own; };
    const OrbmTrackOut L = {or_own(l0.in_view, inl.data()), or_own(l0.proj_x, f.data()), or_own(l0.proj_y, f.data() + M1), or_own(l0.proj_xr, f.data() + 2 * M1),
                            or_own(l0.depth, f.data() + 3 * M1), or_own(l0.view_cos, f.data() + 4 * M1), or_own(l0.scale_level, ll.data())};
    const OrbmTrackOutRight R = {or_own(r0.in_view_r, inr.data()), or_own(r0.proj_xr, f.data() + 5 * M1), or_own(r0.proj_yr, f.data() + 6 * M1),
                                 or_own(r0.depth_r, f.data() + 7 * M1), or_own(r0.view_cos_r, f.data() + 8 * M1), or_own(r0.scale_level_r, lr.data())};
    int rc = orbm_is_in_frustum_rig(h, V, P, cos_limit, &L, &R); if (rc) return rc;
    OrbmMapPointView PV; memset(&PV, 0, sizeof PV);
    PV.M = P->M; PV.in_view = L.in_view; PV.proj_x = L.proj_x; PV.proj_y = L.proj_y; PV.proj_xr = L.proj_xr; PV.scale_level = L.scale_level; PV.view_cos = L.view_cos;
    PV.track_depth = L.depth; PV.is_bad = P->is_bad ? P->is_bad : zero.data(); PV.has_obs = P->has_obs ? P->has_obs : one.data(); PV.desc = P->desc;
    OrbmMapPointRightView PR; PR.in_view_r = R.in_view_r; PR.proj_xr = R.proj_xr; PR.proj_yr = R.proj_yr; PR.scale_level_r = R.scale_level_r; PR.view_cos_r = R.view_cos_r;
    return orbm_search_by_projection_mappoints_fisheye(h, F, &PV, &PR, th, far_points, th_far, nnratio, assigned, nmatches_out);
}

int orbm_search_by_projection_frame_fisheye(orbx_extractor* h, const OrbmFisheyeFrameView* Cur, const OrbmLastFrameView* Last, const float* proj_ur,
                                            const float* proj_vr, float th, int forward, int backward, int check_ori, int* assigned, int* nmatches_out) {
    if (!h || !Cur || !Last || !proj_ur || !proj_vr || !assigned) return fail(ORBX_E_ARG, "null");
    rt::set_device(h->device);
    const int NLast = Last->N, NL = Cur->left.N, NR = Cur->right.N;
    std::vector<AreaQuery> ql(NLast), qr(NLast);
    for (int i = 0; i < NLast; i++) {
        memset(&ql[i], 0, sizeof(AreaQuery)); memset(&qr[i], 0, sizeof(AreaQuery));
        if (!Last->valid[i]) continue;
        const float u = Last->proj_u[i], v = Last->proj_v[i];
        if (u < Cur->left.min_x || u > Cur->left.max_x) continue;          // :2003-2006
        if (v < Cur->left.min_y || v > Cur->left.max_y) continue;
        const int oct = Last->octave[i];
        if (oct < 0 || oct >= Cur->left.nlevels) continue;
        for (int cam = 0; cam < 2; cam++) {
            AreaQuery& q = cam == 0 ? ql[i] : qr[i];
            q.x = cam == 0 ? u : proj_ur[i]; q.y = cam == 0 ? v : proj_vr[i]; q.r = th * Cur->left.scale_factors[oct];
            if (forward) { q.min_level = oct; q.max_level = -1; }
            else if (backward) { q.min_level = 0; q.max_level = oct; }
            else { q.min_level = oct - 1; q.max_level = oct + 1; }
            q.active = 1;
        }
    }
    Csr csl, csr;
    int rc = camera_candidates(h, &Cur->left, ql, Last->desc, &csl); if (rc) return rc;
    rc = camera_candidates(h, &Cur->right, qr, Last->desc, &csr); if (rc) return rc;
    const Cands cl(csl), cr(csr);
    std::vector<uint8_t> occ((size_t)NL + NR + 1, 0);
    if (Cur->left.occupied) memcpy(occ.data(), Cur->left.occupied, NL);
    if (Cur->right.occupied) memcpy(occ.data() + NL, Cur->right.occupied, NR);
    for (int i = 0; i < NL + NR; i++) assigned[i] = -1;
    RotHist hist;
    int nmatches = 0;
    for (int i = 0; i < NLast; i++) {
        if (!ql[i].active || cl.count[i] == 0) continue;                   // an empty left window also skips the right camera (:2025-2026)
        const uint8_t obs = Last->has_obs ? Last->has_obs[i] : 1;
        const Best bl = scan_best(cl, i, occ.data());
        if (bl.dist <= TH_HIGH) {
            assigned[bl.idx] = i; occ[bl.idx] = obs; nmatches++;
            if (check_ori) hist.add(Last->angle[i], Cur->left.keys_un[bl.idx].angle, bl.idx);
        }
        const Best br = scan_best(cr, i, occ.data(), NL);
        if (br.dist <= TH_HIGH) {
            assigned[br.idx + NL] = i; occ[br.idx + NL] = obs; nmatches++;
            if (check_ori) hist.add(Last->angle[i], Cur->right.keys_un[br.idx].angle, br.idx + NL);
        }
    }
    if (check_ori) hist.prune([&](int idx) { assigned[idx] = -2; nmatches--; });
    if (nmatches_out) *nmatches_out = nmatches;
    return ORBX_OK;
}


// ---- the batched rig forms (Tracking::SearchLocalPoints / TrackWithMotionModel with Nleft != -1) ----------------------------------------------
// Frame b = left image lf + b of L's last extraction (camera 1: mvKeys, its descriptors) and right image rf + b of R's (camera 2: mvKeysRight), linked by
// the mvLeftToRightMatch / mvRightToLeftMatch that L's last orbm_stereo_fisheye(L, lf, R, rf, B) left in d_l2r / d_r2l.  One grid per camera per frame
// (Frame::AssignFeaturesToGrid over mvKeys / mvKeysRight, src/Frame.cc:469-504), a window search per camera, the two-camera accept loop of
// k_search.hip (rig_accept_body) one wave per frame; results in L's one pending batch: assigned [B][2 cap] in the slot layout of F.mvpMapPoints.
}  // extern "C"
namespace {
int rig_pair_check(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B) {
    if (!R || B <= 0 || lf < 0 || rf < 0) return fail(ORBX_E_ARG, "bad frame range / null");
    if (lf + B > L->lastB || rf + B > R->lastB)
        return fail(ORBX_E_ARG, "frames [%d, %d) of the left handle / [%d, %d) of the right one exceed their last extractions (%d / %d images)", lf, lf + B, rf, rf + B, L->lastB, R->lastB);
    if (L->kp_total_cap != R->kp_total_cap || L->nlevels != R->nlevels || L->scaleFactor != R->scaleFactor)
        return fail(ORBX_E_ARG, "the two handles differ in orbx_max_keypoints, levels or scale factor");
    if (L->device != R->device) return fail(ORBX_E_ARG, "the two handles sit on different devices");
    if (L->fe_B == 0) return fail(ORBX_E_ARG, "no orbm_stereo_fisheye with this handle on the left: the stereo links of the rig frames are missing");
    if (L->fe_R != R || L->fe_lf != lf || L->fe_rf != rf || L->fe_B != B)
        return fail(ORBX_E_ARG, "the last orbm_stereo_fisheye covered other frames (left %d, right %d, %d pairs)", L->fe_lf, L->fe_rf, L->fe_B);
    if (L->fe_gen_L != L->extract_gen || L->fe_gen_R != R->extract_gen) return fail(ORBX_E_ARG, "a handle has extracted since the last orbm_stereo_fisheye: run it again");
    return ORBX_OK;
}
// the device block of a rig batch behind the upload: two grids, two query sets and CSRs, `extra` bytes of the caller's, the result, the entry pool
struct RigBlock {
    Bump d; GridBlock g1, g2; size_t q1, q2, qs1, qc1, qs2, qc2, extra; ResultBlock r; size_t res, pool;
    RigBlock(size_t o, size_t B1, size_t rows, size_t C1, size_t extra_bytes, bool slot_result = false) : d(o), g1(d, B1, C1), g2(d, B1, C1), r(B1, 2 * C1, slot_result) {       // rows: query rows of the whole batch
        q1 = d.take(sizeof(AreaQuery) * rows); q2 = d.take(sizeof(AreaQuery) * rows);
        qs1 = d.take(4 * rows); qc1 = d.take(4 * rows); qs2 = d.take(4 * rows); qc2 = d.take(4 * rows);
        extra = d.take(extra_bytes); res = d.take(r.bytes); pool = d.o;
    }
};
// grids of both cameras, then the window searches of both query sets into one entry pool (the right-coordinate gate off: a rig frame has no mvuRight)
// queries(): the launch that writes both query sets (and zeroes the pool counter).  maps (device): the table of the frames' query rows and descriptors, M the
// largest of its M_b
template <typename Queries>
void rig_searches(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, int M, const RigBlock& K, uint8_t* dp, const GridParams& g,
                  const FrameMapRec* maps, size_t pool, const Queries& queries) {
    const int cap = L->kp_total_cap;
    const KeyPointRec* kps1 = L->d_kps.p + (size_t)lf * cap; const KeyPointRec* kps2 = R->d_kps.p + (size_t)rf * cap;
    int* d_counter = (int*)(dp + K.res);
    if (L != R) { record_done_if_pending(R); rt::stream_wait_event(L->s0, R->ev_done); }      // the right handle's extraction, before L's stream reads its frames
    if (L->profile) rt::event_record(L->ev_stage[ST_MATCH][0], L->s0);
    {
        dim3 grid(B, 1, 1), blkg(kGridThreads, 1, 1);
        ORBX_LAUNCH(k_grid_build, grid, blkg, 0, L->s0, kps1, 0, g, (int*)(dp + K.g1.cof), (int*)(dp + K.g1.cst), (int*)(dp + K.g1.cit), (const int*)(L->d_nm.p + lf), cap);
        ORBX_LAUNCH(k_grid_build, grid, blkg, 0, L->s0, kps2, 0, g, (int*)(dp + K.g2.cof), (int*)(dp + K.g2.cst), (int*)(dp + K.g2.cit), (const int*)(R->d_nm.p + rf), cap);
    }
    if (M <= 0) { rt::memset_async(d_counter, 0, 16, L->s0); return; }
    queries();
    const float* no_ur = (const float*)dp;                       // never read: gate_right = 0
    dim3 grid((M + 255) / 256, B, 1), blk(256, 1, 1);
    ORBX_LAUNCH(k_area_search_threads, grid, blk, 0, L->s0, (const AreaQuery*)(dp + K.q1), maps, kps1, no_ur, L->d_desc.p + (size_t)lf * cap * 4, g,
                (const int*)(dp + K.g1.cst), (const int*)(dp + K.g1.cit), 0, d_counter, (int)pool, (int*)(dp + K.qs1), (int*)(dp + K.qc1), (int2*)(dp + K.pool), cap);
    ORBX_LAUNCH(k_area_search_threads, grid, blk, 0, L->s0, (const AreaQuery*)(dp + K.q2), maps, kps2, no_ur, R->d_desc.p + (size_t)rf * cap * 4, g,
                (const int*)(dp + K.g2.cst), (const int*)(dp + K.g2.cit), 0, d_counter, (int)pool, (int*)(dp + K.qs2), (int*)(dp + K.qc2), (int2*)(dp + K.pool), cap);
}
size_t rig_accept_lds(int cap, int events) { const size_t S = 2 * (size_t)cap; return 4 * S + al16(S) + 4 * (size_t)events + 64; }
// orbm_search_local_points_rig_batch (one resident set, `maps` == NULL) and orbm_search_local_points_rig_batch_maps (maps[b] = frame b's own)
int local_points_rig_batch(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const OrbmFrustumRigView* frames, const orbm_points* points,
                           const uint8_t* is_bad, const uint8_t* has_obs, const OrbmFrameMap* maps, const uint8_t* occupied, float cos_limit, float th, int far_points,
                           float th_far, float nnratio, int want_in_view, const MapSetRec* sets = nullptr) {
    if (!L || !frames || (!points && !maps && !sets)) return fail(ORBX_E_ARG, "null");
    int rc = rig_pair_check(L, lf, R, rf, B); if (rc) return rc;
    if ((rc = frames_check(&frames[0].left, sizeof *frames, B))) return rc;
    BatchMaps P{points, is_bad, has_obs, maps, B, sets};
    if ((rc = P.plan(L->device))) return rc;
    rt::set_device(L->device);
    const int M = P.m_max, cap = L->kp_total_cap;
    const size_t B1 = B, C1 = cap, S1 = 2 * C1, rows = P.rows;
    const size_t smem_accept = rig_accept_lds(cap, 0);
    if (smem_accept + 1024 > rt::lds_limit(L->device)) return fail(ORBX_E_CAPACITY, "%d keypoints per camera need %zu bytes of LDS in the rig accept kernel", cap, smem_accept);
    // upload: [camera 1, camera 2] parameters per frame | the table of per-frame maps | bad flags | has-observation flags | occupancy [B][2 cap]
    // (on a map's own sets: the table of k_map_set_flags in place of the flags, which lie behind the upload - as local_points_batch)
    Bump u;
    const size_t u_f = u.take(sizeof(FrustumParams) * 2 * B1), u_tab = u.take(P.table_bytes()), up_bad = u.take(sets ? 0 : P.flags), up_obs = u.take(sets ? 0 : P.flags),
                 u_occ = u.take(occupied ? B1 * S1 : 0), u_ftab = u.take(P.flag_table_bytes()), u_total = u.o;
    Bump behind(u_total);
    const size_t u_bad = sets ? behind.take(P.flags) : up_bad, u_obs = sets ? behind.take(P.flags) : up_obs;
    // behind the common block: per camera track [5 rows] | level [rows] | in_view [rows]   (rows: the sum of the frames' M_b; B x M for one set)
    Bump t;
    const size_t o_trk1 = t.take(20 * rows), o_trk2 = t.take(20 * rows), o_lvl1 = t.take(4 * rows), o_lvl2 = t.take(4 * rows), o_view1 = t.take(rows), o_view2 = t.take(rows);
    const RigBlock K(behind.o, B1, rows, C1, t.o, sets != nullptr);
    const size_t pool = batch_pool(L, rows * 12 + 4096);
    if (!batch_reserve(L, K.pool, pool, u_total, al16(K.r.bytes) + (want_in_view ? 2 * rows : 0)))
        return fail(ORBX_E_DEVICE, "allocation failed (batched rig local point search, %d frames, %zu points)", B, rows);
    uint8_t* hp = L->h_lp_in.p; uint8_t* dp = L->d_lp.p; uint8_t* dx = dp + K.extra;
    FrustumParams* Fp = (FrustumParams*)(hp + u_f);
    for (int b = 0; b < B; b++) {
        fill_frustum_params(&frames[b].left, cos_limit, th, far_points, th_far, &Fp[2 * b]); Fp[2 * b].rig_mode = 1;
        right_camera_params(&frames[b], cos_limit, &Fp[2 * b + 1]);
    }
    P.stage(hp + u_tab, hp + up_bad, hp + up_obs);
    if (sets) P.flag_table(hp + u_ftab);
    if (occupied) memcpy(hp + u_occ, occupied, B1 * S1);
    if ((rc = batch_upload(L, u_total, nullptr, B, M))) return rc;
    if (sets) P.gather_flags(L->s0, dp + u_ftab, dp + u_bad, dp + u_obs);
    const FrameMapRec* d_tab = (const FrameMapRec*)(dp + u_tab);
    rig_searches(L, lf, R, rf, B, M, K, dp, grid_from_view(frames[0].left), d_tab, pool, [&]() {
        dim3 grid((M + 255) / 256, B, 1), blk(256, 1, 1);
        ORBX_LAUNCH(k_frustum_rig, grid, blk, 0, L->s0, (const FrustumParams*)(dp + u_f), d_tab, (const uint8_t*)(dp + u_bad), dx + o_view1, dx + o_view2,
                    (float*)(dx + o_trk1), (float*)(dx + o_trk2), (int*)(dx + o_lvl1), (int*)(dx + o_lvl2), (AreaQuery*)(dp + K.q1), (AreaQuery*)(dp + K.q2),
                    (int*)(dp + K.res));
    });
    {
        dim3 grid(B, 1, 1), blk(64, 1, 1);
        const uint8_t* d_occ = occupied ? (const uint8_t*)(dp + u_occ) : (const uint8_t*)nullptr;
        ORBX_LAUNCH(k_rig_local_accept, grid, blk, smem_accept, L->s0, d_tab, cap, (const int*)(L->d_nm.p + lf), (const int*)(R->d_nm.p + rf), (const int*)(dp + K.qs1),
                    (const int*)(dp + K.qc1), (const int*)(dp + K.qs2), (const int*)(dp + K.qc2), (const int2*)(dp + K.pool), d_occ, (const uint8_t*)(dp + u_obs),
                    (const int*)L->d_l2r.p, (const int*)L->d_r2l.p, nnratio, TH_HIGH, (int*)(dp + K.res + K.r.assigned), (int*)(dp + K.res + K.r.nmatches));
    }
    if (sets) P.translate(L->s0, dp + u_ftab, (const int*)(dp + K.res + K.r.assigned), 2 * cap, (int*)(dp + K.res + K.r.as_slots));
    return batch_finish(L, {B, M, P.M, K.res, {K.extra + o_view1, K.extra + o_view2}, want_in_view != 0, true, sets != nullptr});
}
}  // namespace
extern "C" {

int orbm_search_local_points_rig_batch(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const OrbmFrustumRigView* frames, const orbm_points* points,
                                       const uint8_t* is_bad, const uint8_t* has_obs, const uint8_t* occupied, float cos_limit, float th, int far_points,
                                       float th_far, float nnratio, int want_in_view) {
    batch_clear(L);
    return local_points_rig_batch(L, lf, R, rf, B, frames, points, is_bad, has_obs, nullptr, occupied, cos_limit, th, far_points, th_far, nnratio, want_in_view);
}

int orbm_search_local_points_rig_batch_maps(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const OrbmFrustumRigView* frames, const OrbmFrameMap* maps,
                                            const uint8_t* occupied, float cos_limit, float th, int far_points, float th_far, float nnratio, int want_in_view) {
    batch_clear(L);
    if (L && !maps) return fail(ORBX_E_ARG, "null table of per-frame maps");
    return local_points_rig_batch(L, lf, R, rf, B, frames, nullptr, nullptr, nullptr, maps, occupied, cos_limit, th, far_points, th_far, nnratio, want_in_view);
}

// orbm_search_by_projection_lastframe_rig_batch (src == nullptr: the rows are the caller's arrays) and .._rig_batch_map (the rows are read from the map,
// whose mutex the caller holds until this returns).  The entry points have checked their own arguments (L among them) and cleared the pending batch
static int lastframe_rig_batch(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const OrbmFrustumRigView* cur, const float* trl, const PointRows* last,
                               const MapRows* src, float th, const uint8_t* forward, const uint8_t* backward, int check_ori, const uint8_t* occupied) {
    int rc = rig_pair_check(L, lf, R, rf, B); if (rc) return rc;
    if ((rc = frames_check(&cur[0].left, sizeof *cur, B))) return rc;
    const int M = last->cap, cap = L->kp_total_cap;
    for (int b = 0; b < B; b++) if (last->n[b] < 0 || last->n[b] > M) return fail(ORBX_E_ARG, "frame %d: %d points in %d rows", b, last->n[b], M);
    rt::set_device(L->device);
    const size_t B1 = B, M1 = M, C1 = cap, S1 = 2 * C1;
    const size_t smem_accept = rig_accept_lds(cap, 2 * M);     // grows with cap_last: checked before anything is enqueued
    if (smem_accept + 1024 > rt::lds_limit(L->device))
        return fail(ORBX_E_CAPACITY, "%d keypoints per camera and %d last-frame points per frame need %zu bytes of LDS in the rig accept kernel", cap, M, smem_accept);
    // upload: camera-1 parameters per frame | the table of the frames' rows | n_last | pos | valid | octave | angle | has_obs | descriptors | occupancy [B][2 cap]
    Bump u;
    const size_t u_f = u.take(sizeof(FrustumParams) * B1), u_tab = u.take(sizeof(FrameMapRec) * B1);
    PointRowsUpload U(u, B1, M1, src, false);
    const size_t u_occ = u.take(occupied ? B1 * S1 : 0), u_total = u.o;
    Bump behind(u_total);
    U.device_rows(behind, B1, M1);                              // (map-fed: the gathered rows between the upload and the rig block)
    const RigBlock K(behind.o, B1, B1 * M1, C1, 0);
    const size_t pool = batch_pool(L, B1 * M1 * 32 + 4096);                    // th = 7 .. 15 px windows, two cameras
    if (!batch_reserve(L, K.pool, pool, u_total, al16(K.r.bytes)))
        return fail(ORBX_E_DEVICE, "allocation failed (batched rig last-frame search, %d frames x %d points)", B, M);
    uint8_t* hp = L->h_lp_in.p; uint8_t* dp = L->d_lp.p;
    FrustumParams* Fp = (FrustumParams*)(hp + u_f);
    for (int b = 0; b < B; b++) {
        fill_frustum_params(&cur[b].left, 0.0f, th, 0, 0.0f, &Fp[b]);
        Fp[b].forward = forward ? forward[b] != 0 : 0; Fp[b].backward = backward ? backward[b] != 0 : 0; Fp[b].debug_flags = L->debug_stereo_flags;
    }
    U.stage(hp, *last, B1, M1);
    stage_uniform_table(hp + u_tab, B, M, (const unsigned long long*)(dp + U.u_desc));
    if (occupied) memcpy(hp + u_occ, occupied, B1 * S1);
    if ((rc = batch_upload(L, u_total, &U, B, M))) return rc;
    RigRelPose T; memcpy(T.q, trl, sizeof T.q); memcpy(T.t, trl + 4, sizeof T.t);
    const FrameMapRec* d_tab = (const FrameMapRec*)(dp + u_tab);
    rig_searches(L, lf, R, rf, B, M, K, dp, grid_from_view(cur[0].left), d_tab, pool, [&]() {
        dim3 grid((M + 255) / 256, B, 1), blk(256, 1, 1);
        ORBX_LAUNCH(k_lastframe_queries_rig, grid, blk, 0, L->s0, (const FrustumParams*)(dp + u_f), M, (const int*)(dp + U.u_n), (const float*)(dp + U.u_pos),
                    (const uint8_t*)(dp + U.u_val), (const int*)(dp + U.u_oct), T, (AreaQuery*)(dp + K.q1), (AreaQuery*)(dp + K.q2), (int*)(dp + K.res));
    });
    {
        dim3 grid(B, 1, 1), blk(64, 1, 1);
        ORBX_LAUNCH(k_rig_lastframe_accept, grid, blk, smem_accept, L->s0, d_tab, cap, (const int*)(L->d_nm.p + lf), (const int*)(R->d_nm.p + rf), (const int*)(dp + K.qs1),
                    (const int*)(dp + K.qc1), (const int*)(dp + K.qs2), (const int*)(dp + K.qc2), (const int2*)(dp + K.pool),
                    occupied ? (const uint8_t*)(dp + u_occ) : (const uint8_t*)nullptr, (const uint8_t*)(dp + U.u_obs), TH_HIGH, (int*)(dp + K.res + K.r.assigned),
                    (int*)(dp + K.res + K.r.nmatches), (const float*)(dp + U.u_ang), (const KeyPointRec*)(L->d_kps.p + (size_t)lf * cap), (const KeyPointRec*)(R->d_kps.p + (size_t)rf * cap),
                    check_ori);
    }
    return batch_finish(L, {B, M, {}, K.res, {0, 0}, false, true});
}

int orbm_search_by_projection_lastframe_rig_batch(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const OrbmFrustumRigView* cur, const float* trl,
                                                  const OrbmLastFrameBatch* last, float th, const uint8_t* forward, const uint8_t* backward, int check_ori,
                                                  const uint8_t* occupied) {
    batch_clear(L);
    if (!L || !cur || !trl || !last) return fail(ORBX_E_ARG, "null");
    if (last->cap_last <= 0 || !last->n || !last->pos || !last->valid || !last->octave || !last->angle || !last->desc) return fail(ORBX_E_ARG, "bad last-frame batch");
    const PointRows rows = last_frame_rows(last);
    return lastframe_rig_batch(L, lf, R, rf, B, cur, trl, &rows, nullptr, th, forward, backward, check_ori, occupied);
}

int orbm_search_rig_batch_fetch(orbx_extractor* L, int* assigned, int cap, int* nmatches, uint8_t* in_view, uint8_t* in_view_r) {
    if (!L || L->batch.B <= 0 || !L->batch.rig) return fail(ORBX_E_ARG, "no batched rig search is pending");
    if (assigned && cap < 2 * L->kp_total_cap) return fail(ORBX_E_ARG, "assigned rows need %d entries (2 x orbx_max_keypoints)", 2 * L->kp_total_cap);
    if ((in_view || in_view_r) && !L->batch.want_view) return fail(ORBX_E_ARG, "in_view was not requested at enqueue time");
    uint8_t* const views[2] = {in_view, in_view_r};
    return batch_fetch(L, 2 * (size_t)L->kp_total_cap, "batched rig search", assigned, cap, nmatches, 2, L->batch.want_view && L->batch.M > 0, views);
}

}  // extern "C"

// ---- the resident map: map points by slot, key-frame rows of slots, Tracking::UpdateLocalPoints on the device -----------------------------------
// What the searches read of a map point changes where LocalMapping / LoopClosing touch it; WHICH points a frame's local map lists, and in what order,
// changes every frame (Tracking::UpdateLocalPoints rebuilds mvpLocalMapPoints from scratch, src/Tracking.cc:4088-4120).  So the fields live in a store
// addressed by slot, GetMapPointMatches() of every key frame is a row of slots, and the list of a frame - rows walked in the caller's order, the first
// occurrence of every good point kept - is built by the kernels k_map_* into an orbm_points set the map owns.  Every call takes the map's mutex and
// waits for its own work, so handles of different threads (LocalMapping's, Tracking's) may share a map.  The searches that read their rows from the map
// (the .._batch_map calls at the end of this file) hold the mutex until the event behind their gather has passed and leave the rest of the search running:
// what they read of the map is copied by then.
// Lock order: a call that needs the vocabulary's lock (orbv_lock) and a map's mutex takes the vocabulary's FIRST (orbm_search_by_bow_frames_batch_map and
// orbm_search_by_bow_rig_batch_map); no call holds two maps' mutexes.  kf_grid_mutex() is taken AFTER a map's mutex where both are needed
// (orbm_fuse_candidates_batch_map, orbm_search_by_projection_sim3_batch_map), never the other way round, and never together with the vocabulary's.
struct orbm_map {
    int device = 0, slots = 0, kf_rows = 0, kf_row_cap = 0, max_sets = 0;
    mutable std::mutex mu;
    DevBuf<uint8_t> d_store; MapStore S = {};      // [descriptors 32 | pos 12 | normal 12 | min 4 | max 4 | state 1] x slots
    DevBuf<int> d_kf;                              // [kf_rows][kf_row_cap] slots; the rows' lengths stay on the host
    DevBuf<unsigned> d_stamp;                      // [max_sets][slots] first-occurrence stamps, then [max_sets][slots] seen stamps
    std::vector<int> kf_n; std::vector<uint8_t> kf_set;     // (kf_set: orbm_map_set_keyframe has written the row)
    std::vector<uint8_t> state, mark;              // host mirror of S.state (what orbm_map_select checks); scratch of the duplicate check
    // stamps of one build lie in (base, base + its largest position count]; base then moves up, and everything older reads as stale.  At epoch_limit
    // (orbm_map_debug_epoch: tests lower it) the stamps are cleared and base starts over
    unsigned base = 0, epoch_limit = 0xFFFFFFFFu;
    // [slots] "which position of the set is this slot" of the Fuse / Sim3 batches fed from the map (k_map_set_table), allocated by the first of them; a
    // call's entries lie in (tbase, tbase + M] and tbase then moves up, as `base` does (the same epoch_limit; map_skip_table)
    DevBuf<unsigned> d_table; unsigned tbase = 0;
    std::vector<orbm_points> sets; std::vector<DevBuf<uint8_t>> set_mem; std::vector<MapSetRec> set_rec; std::vector<uint8_t> built;
    HostBuf<uint8_t> h_stage; DevBuf<uint8_t> d_stage;      // one call's upload, counts and set table (the mutex makes them the call's own)
};

namespace {
int map_call_check(const orbx_extractor* h, const orbm_map* m) {
    if (!h || !m) return fail(ORBX_E_ARG, "null handle or map");
    if (h->device != m->device) return fail(ORBX_E_ARG, "the map lives on device %d, the handle on device %d", m->device, h->device);
    return ORBX_OK;
}
int map_stage(orbm_map* m, size_t host_bytes, size_t dev_bytes) {
    if (m->h_stage.ensure(host_bytes + 16) || m->d_stage.ensure(dev_bytes + 16)) return fail(ORBX_E_DEVICE, "staging allocation failed");
    return ORBX_OK;
}
// set b laid out for M points in memory that only grows: [descriptors | pos | normal | min | max | slots | seen]; the set reads as empty until its build has ended
int map_lay_set(orbm_map* m, int b, int M) {
    const size_t M1 = M > 0 ? M : 1;
    Bump L;
    const size_t od = L.take(32 * M1), op = L.take(12 * M1), on = L.take(12 * M1), omn = L.take(4 * M1), omx = L.take(4 * M1), osl = L.take(4 * M1), ose = L.take(M1);
    orbm_points& P = m->sets[b];
    P.M = 0;
    if (m->set_mem[b].ensure(L.o)) return fail(ORBX_E_DEVICE, "set %d: allocation for %d points failed", b, M);
    uint8_t* p = m->set_mem[b].p;
    MapSetRec& R = m->set_rec[b];
    R.desc = (unsigned long long*)(p + od); R.pos = (float*)(p + op); R.normal = (float*)(p + on); R.min_d = (float*)(p + omn); R.max_d = (float*)(p + omx);
    R.slots = (int*)(p + osl); R.seen = p + ose; R.M = M; R.set = b;
    P.device = m->device; P.dmem = p; P.desc = R.desc; P.pos = R.pos; P.normal = R.normal; P.min_d = R.min_d; P.max_d = R.max_d; P.map_owned = true;
    m->built[b] = 1;
    return ORBX_OK;
}
// n slots of the map, each once (a parallel scatter must not meet itself)
int map_distinct_slots(orbm_map* m, int n, const int* slots) {
    int rc = ORBX_OK, i = 0;
    for (; i < n; i++) {
        const int s = slots[i];
        if (s < 0 || s >= m->slots) { rc = fail(ORBX_E_ARG, "entry %d: slot %d is outside the map's %d slots", i, s, m->slots); break; }
        if (m->mark[s]) { rc = fail(ORBX_E_ARG, "entry %d: slot %d is listed twice", i, s); break; }
        m->mark[s] = 1;
    }
    for (int k = 0; k < i; k++) m->mark[slots[k]] = 0;
    return rc;
}
// orbm_map_update (P != nullptr) and orbm_map_set_bad: one staged block up, one launch
int map_scatter(orbx_extractor* h, orbm_map* m, int n, const int* slots, const OrbmWorldPointView* P, const uint8_t* bad) {
    const size_t N = n;
    Bump L;
    const size_t os = L.take(4 * N), ob = L.take(N), od = L.take(P ? 32 * N : 0), op = L.take(P ? 12 * N : 0), on = L.take(P ? 12 * N : 0), omn = L.take(P ? 4 * N : 0),
                 omx = L.take(P ? 4 * N : 0);
    if (int rc = map_stage(m, L.o, L.o)) return rc;
    uint8_t* hp = m->h_stage.p; uint8_t* dp = m->d_stage.p;
    memcpy(hp + os, slots, 4 * N);
    if (bad) memcpy(hp + ob, bad, N); else memset(hp + ob, 0, N);
    if (P) { memcpy(hp + od, P->desc, 32 * N); memcpy(hp + op, P->pos, 12 * N); memcpy(hp + on, P->normal, 12 * N); memcpy(hp + omn, P->min_distance, 4 * N); memcpy(hp + omx, P->max_distance, 4 * N); }
    if (rt::copy_h2d(dp, hp, L.o, h->s0)) return fail(ORBX_E_DEVICE, "upload failed: %s", rt::last_error());
    const dim3 grid((unsigned)((4 * N + 255) / 256), 1, 1), blk(256, 1, 1);
    ORBX_LAUNCH(k_map_scatter, grid, blk, 0, h->s0, n, (const int*)(dp + os), P ? (const unsigned long long*)(dp + od) : (const unsigned long long*)nullptr, (const float*)(dp + op),
                (const float*)(dp + on), (const float*)(dp + omn), (const float*)(dp + omx), (const uint8_t*)(dp + ob), m->S);
    if (rt::stream_sync(h->s0) || rt::check_launch()) return fail(ORBX_E_DEVICE, "map update failed: %s", rt::last_error());
    for (int i = 0; i < n; i++) {
        const uint8_t st = (uint8_t)(kMapPresent | (bad && bad[i] ? kMapBad : 0));
        if (P || (m->state[slots[i]] & kMapPresent)) m->state[slots[i]] = st;
    }
    return ORBX_OK;
}
void map_release(orbm_map* m) {
    m->d_store.release(); m->d_kf.release(); m->d_stamp.release(); m->d_table.release(); m->h_stage.release(); m->d_stage.release();
    for (auto& x : m->set_mem) x.release();
}
}  // namespace

extern "C" {

int orbm_map_create(orbx_extractor* h, int slots, int kf_rows, int kf_row_cap, int max_sets, orbm_map** out) {
    if (!h || !out) return fail(ORBX_E_ARG, "null");
    if (slots < 1 || kf_rows < 0 || kf_row_cap < 0 || max_sets < 1) return fail(ORBX_E_ARG, "a map needs slots >= 1, kf_rows >= 0, kf_row_cap >= 0, max_sets >= 1");
    if (slots > (1 << 28) || max_sets > 65535 || kf_row_cap > (1 << 22) || (long long)kf_rows * kf_row_cap > (1ll << 30) || (long long)max_sets * slots > (1ll << 31))
        return fail(ORBX_E_CAPACITY, "at most 2^28 slots, 65535 sets, rows of 2^22, 2^30 row entries and 2^31 (set, slot) pairs");
    rt::set_device(h->device);
    orbm_map* m = new orbm_map();
    m->device = h->device; m->slots = slots; m->kf_rows = kf_rows; m->kf_row_cap = kf_row_cap; m->max_sets = max_sets;
    const size_t S1 = slots, pairs = (size_t)max_sets * S1;
    Bump L;
    const size_t od = L.take(32 * S1), op = L.take(12 * S1), on = L.take(12 * S1), omn = L.take(4 * S1), omx = L.take(4 * S1), ost = L.take(S1);
    if (m->d_store.ensure(L.o) || m->d_kf.ensure((size_t)kf_rows * kf_row_cap + 1) || m->d_stamp.ensure(2 * pairs) ||
        rt::memset_async(m->d_store.p, 0, L.o, h->s0) || rt::memset_async(m->d_stamp.p, 0, 2 * pairs * sizeof(unsigned), h->s0) || rt::stream_sync(h->s0)) {
        map_release(m); delete m;
        return fail(ORBX_E_DEVICE, "allocation of a map of %d slots, %d x %d row entries and %d sets failed", slots, kf_rows, kf_row_cap, max_sets);
    }
    uint8_t* p = m->d_store.p;
    m->S.desc = (unsigned long long*)(p + od); m->S.pos = (float*)(p + op); m->S.normal = (float*)(p + on); m->S.min_d = (float*)(p + omn); m->S.max_d = (float*)(p + omx);
    m->S.state = p + ost;
    m->kf_n.assign(kf_rows, 0); m->kf_set.assign(kf_rows, 0); m->state.assign(S1, 0); m->mark.assign(S1, 0);
    m->sets.resize(max_sets); m->set_mem.resize(max_sets); m->set_rec.resize(max_sets); m->built.assign(max_sets, 0);
    *out = m;
    return ORBX_OK;
}

int orbm_map_destroy(orbx_extractor* /*h*/, orbm_map* m) {
    if (!m) return ORBX_OK;
    rt::set_device(m->device);
    map_release(m);
    delete m;
    return ORBX_OK;
}

int orbm_map_debug_epoch(orbx_extractor* h, orbm_map* m, int limit) {
    if (int rc = map_call_check(h, m)) return rc;
    std::lock_guard<std::mutex> lk(m->mu);
    rt::set_device(h->device);
    if (rt::memset_async(m->d_stamp.p, 0, 2 * (size_t)m->max_sets * m->slots * sizeof(unsigned), h->s0) ||
        (m->d_table.p && rt::memset_async(m->d_table.p, 0, (size_t)m->slots * sizeof(unsigned), h->s0)) || rt::stream_sync(h->s0))
        return fail(ORBX_E_DEVICE, "clearing the stamps failed");
    m->base = 0; m->tbase = 0; m->epoch_limit = limit > 0 ? (unsigned)limit : 0xFFFFFFFFu;
    return ORBX_OK;
}

int orbm_map_update(orbx_extractor* h, orbm_map* m, int n, const int* slots, const OrbmWorldPointView* P) {
    if (int rc = map_call_check(h, m)) return rc;
    if (n < 0) return fail(ORBX_E_ARG, "negative number of points");
    if (n == 0) return ORBX_OK;
    if (!slots || !P || P->M != n || !P->pos || !P->normal || !P->min_distance || !P->max_distance || !P->desc) return fail(ORBX_E_ARG, "bad map point view (M has to be n, every field present)");
    std::lock_guard<std::mutex> lk(m->mu);
    if (int rc = map_distinct_slots(m, n, slots)) return rc;
    rt::set_device(h->device);
    return map_scatter(h, m, n, slots, P, P->is_bad);
}

int orbm_map_set_bad(orbx_extractor* h, orbm_map* m, int n, const int* slots, const uint8_t* bad) {
    if (int rc = map_call_check(h, m)) return rc;
    if (n < 0) return fail(ORBX_E_ARG, "negative number of points");
    if (n == 0) return ORBX_OK;
    if (!slots || !bad) return fail(ORBX_E_ARG, "null");
    std::lock_guard<std::mutex> lk(m->mu);
    if (int rc = map_distinct_slots(m, n, slots)) return rc;
    rt::set_device(h->device);
    return map_scatter(h, m, n, slots, nullptr, bad);
}

int orbm_map_set_keyframe(orbx_extractor* h, orbm_map* m, int row, int n, const int* slots) {
    if (int rc = map_call_check(h, m)) return rc;
    if (row < 0 || row >= m->kf_rows) return fail(ORBX_E_ARG, "row %d is outside the map's %d key-frame rows", row, m->kf_rows);
    if (n < 0 || (n > 0 && !slots)) return fail(ORBX_E_ARG, "row %d: null / negative number of features", row);
    if (n > m->kf_row_cap) return fail(ORBX_E_CAPACITY, "row %d: %d features, the map's rows hold %d", row, n, m->kf_row_cap);
    for (int i = 0; i < n; i++)
        if (slots[i] < -1 || slots[i] >= m->slots) return fail(ORBX_E_ARG, "row %d: slot %d of feature %d is outside the map's %d slots", row, slots[i], i, m->slots);
    std::lock_guard<std::mutex> lk(m->mu);
    rt::set_device(h->device);
    if (n > 0) {
        if (int rc = map_stage(m, 4 * (size_t)n, 0)) return rc;
        memcpy(m->h_stage.p, slots, 4 * (size_t)n);
        if (rt::copy_h2d(m->d_kf.p + (size_t)row * m->kf_row_cap, m->h_stage.p, 4 * (size_t)n, h->s0) || rt::stream_sync(h->s0)) return fail(ORBX_E_DEVICE, "row %d: upload failed: %s", row, rt::last_error());
    }
    m->kf_n[row] = n; m->kf_set[row] = 1;
    return ORBX_OK;
}

int orbm_map_local_points(orbx_extractor* h, orbm_map* m, int B, const int* kf_start, const int* kf_rows, const int* seen_start, const int* seen_slots, int* M_out) {
    if (int rc = map_call_check(h, m)) return rc;
    if (B < 0) return fail(ORBX_E_ARG, "negative number of frames");
    if (B == 0) return ORBX_OK;
    if (!kf_start || !M_out) return fail(ORBX_E_ARG, "null");
    if (B > m->max_sets) return fail(ORBX_E_CAPACITY, "%d frames, the map has %d sets", B, m->max_sets);
    std::lock_guard<std::mutex> lk(m->mu);
    // the walk of every frame as segments (one per visited row) and chunks of kMapChunk positions; everything is checked before anything is enqueued
    const long long max_positions = std::min<long long>(0x7fffffff, m->epoch_limit);
    std::vector<MapSeg> segs; std::vector<int> fc0(B + 1); std::vector<long long> P(B);
    long long nchunks = 0, L = 0; int max_n = 0;
    if (kf_start[0] < 0) return fail(ORBX_E_ARG, "frame 0: negative kf_start");
    for (int b = 0; b < B; b++) {
        if (kf_start[b + 1] < kf_start[b]) return fail(ORBX_E_ARG, "frame %d: kf_start decreases", b);
        if (kf_start[b + 1] > kf_start[b] && !kf_rows) return fail(ORBX_E_ARG, "frame %d: null row list", b);
        fc0[b] = (int)nchunks;
        long long p = 0;
        for (int k = kf_start[b]; k < kf_start[b + 1]; k++) {
            const int row = kf_rows[k];
            if (row < 0 || row >= m->kf_rows) return fail(ORBX_E_ARG, "frame %d: row %d is outside the map's %d key-frame rows", b, row, m->kf_rows);
            const int n = m->kf_n[row];
            if (p + n > max_positions) return fail(ORBX_E_CAPACITY, "frame %d visits more than %lld positions", b, max_positions);
            const MapSeg g = {b, row, n, (int)p, (int)nchunks};
            segs.push_back(g);
            p += n; nchunks += (n + kMapChunk - 1) / kMapChunk; max_n = std::max(max_n, n);
            if (nchunks > (1ll << 30) || segs.size() > ((size_t)1 << 24)) return fail(ORBX_E_CAPACITY, "frame %d: more than 2^30 chunks or 2^24 visited rows in one call", b);
        }
        P[b] = p; L = std::max(L, p);
    }
    fc0[B] = (int)nchunks;
    int seen_total = 0, max_seen = 0;
    if (seen_start) {
        if (seen_start[0] < 0) return fail(ORBX_E_ARG, "frame 0: negative seen_start");
        for (int b = 0; b < B; b++) {
            if (seen_start[b + 1] < seen_start[b]) return fail(ORBX_E_ARG, "frame %d: seen_start decreases", b);
            if (seen_start[b + 1] > seen_start[b] && !seen_slots) return fail(ORBX_E_ARG, "frame %d: null seen list", b);
            for (int k = seen_start[b]; k < seen_start[b + 1]; k++)
                if (seen_slots[k] < 0 || seen_slots[k] >= m->slots) return fail(ORBX_E_ARG, "frame %d: seen slot %d is outside the map's %d slots", b, seen_slots[k], m->slots);
            max_seen = std::max(max_seen, seen_start[b + 1] - seen_start[b]);
        }
        seen_total = seen_start[B];
    }
    rt::set_device(h->device);
    for (int b = 0; b < B; b++) m->sets[b].M = 0;
    if (L == 0) {                                                   // nothing is visited: every local map is empty
        for (int b = 0; b < B; b++) { if (int rc = map_lay_set(m, b, 0)) return rc; M_out[b] = 0; }
        return ORBX_OK;
    }
    const size_t nseg = segs.size(), B1 = B;
    Bump U;
    const size_t o_seg = U.take(sizeof(MapSeg) * nseg), o_fc0 = U.take(4 * (B1 + 1)), o_ss = U.take(4 * (B1 + 1)), o_sl = U.take(4 * (size_t)seen_total), up = U.o;
    const size_t o_cnt = U.take(4 * (size_t)nchunks), o_off = U.take(4 * (size_t)nchunks), o_M = U.take(4 * B1), o_tab = U.take(sizeof(MapSetRec) * B1);
    const size_t h_M = up, h_tab = up + al16(4 * B1);
    if (int rc = map_stage(m, h_tab + sizeof(MapSetRec) * B1, U.o)) return rc;
    uint8_t* hp = m->h_stage.p; uint8_t* dp = m->d_stage.p;
    memcpy(hp + o_seg, segs.data(), sizeof(MapSeg) * nseg); memcpy(hp + o_fc0, fc0.data(), 4 * (B1 + 1));
    if (max_seen > 0) { memcpy(hp + o_ss, seen_start, 4 * (B1 + 1)); memcpy(hp + o_sl, seen_slots, 4 * (size_t)seen_total); }
    const size_t pairs = (size_t)m->max_sets * m->slots;
    unsigned* stamp = m->d_stamp.p; unsigned* seen_stamp = stamp + pairs;
    if ((long long)m->base + L > (long long)m->epoch_limit) {       // the epoch is used up: clear, start over
        if (rt::memset_async(stamp, 0, 2 * pairs * sizeof(unsigned), h->s0)) return fail(ORBX_E_DEVICE, "clearing the stamps failed: %s", rt::last_error());
        m->base = 0;
    }
    const unsigned base = m->base, top = base + (unsigned)L;
    m->base = top;                                                  // (whatever happens from here on, the stamps this call leaves are stale for the next one)
    if (rt::copy_h2d(dp, hp, up, h->s0)) return fail(ORBX_E_DEVICE, "upload failed: %s", rt::last_error());
    const MapSeg* d_seg = (const MapSeg*)(dp + o_seg);
    if (max_seen > 0) {
        const dim3 grid((max_seen + 255) / 256, B, 1), blk(256, 1, 1);
        ORBX_LAUNCH(k_map_seen, grid, blk, 0, h->s0, (const int*)(dp + o_ss), (const int*)(dp + o_sl), seen_stamp, m->slots, base + 1u);
    }
    const dim3 gridp((unsigned)nseg, (max_n + kMapChunk - 1) / kMapChunk, 1), blkp(kMapChunk, 1, 1), gridb(B, 1, 1), wave(64, 1, 1);
    ORBX_LAUNCH(k_map_stamp, gridp, blkp, 0, h->s0, d_seg, (const int*)m->d_kf.p, m->kf_row_cap, (const uint8_t*)m->S.state, stamp, m->slots, top);
    ORBX_LAUNCH(k_map_compact, gridp, blkp, 0, h->s0, d_seg, (const int*)m->d_kf.p, m->kf_row_cap, (const uint8_t*)m->S.state, (const unsigned*)stamp, m->slots, top,
                (int*)(dp + o_cnt), (const int*)nullptr, (const MapSetRec*)nullptr);
    ORBX_LAUNCH(k_map_scan, gridb, wave, 0, h->s0, (const int*)(dp + o_fc0), (const int*)(dp + o_cnt), (int*)(dp + o_off), (int*)(dp + o_M));
    if (rt::copy_d2h(hp + h_M, dp + o_M, 4 * B1, h->s0) || rt::stream_sync(h->s0) || rt::check_launch()) return fail(ORBX_E_DEVICE, "local map build failed: %s", rt::last_error());
    // the sizes are known: lay the sets out, scatter the kept slots in visiting order, gather the fields
    const int* Mb = (const int*)(hp + h_M);
    int m_max = 0;
    for (int b = 0; b < B; b++) {
        if (Mb[b] < 0 || Mb[b] > P[b] || Mb[b] > m->slots) return fail(ORBX_E_INTERNAL, "frame %d: %d kept of %lld visited positions", b, Mb[b], P[b]);
        if (int rc = map_lay_set(m, b, Mb[b])) return rc;
        m_max = std::max(m_max, Mb[b]);
    }
    memcpy(hp + h_tab, m->set_rec.data(), sizeof(MapSetRec) * B1);
    if (rt::copy_h2d(dp + o_tab, hp + h_tab, sizeof(MapSetRec) * B1, h->s0)) return fail(ORBX_E_DEVICE, "upload failed: %s", rt::last_error());
    if (m_max > 0) {
        const MapSetRec* d_tab = (const MapSetRec*)(dp + o_tab);
        ORBX_LAUNCH(k_map_compact, gridp, blkp, 0, h->s0, d_seg, (const int*)m->d_kf.p, m->kf_row_cap, (const uint8_t*)m->S.state, (const unsigned*)stamp, m->slots, top,
                    (int*)(dp + o_cnt), (const int*)(dp + o_off), d_tab);
        const dim3 gridg((unsigned)((4 * (size_t)m_max + 255) / 256), B, 1), blkg(256, 1, 1);
        ORBX_LAUNCH(k_map_gather, gridg, blkg, 0, h->s0, d_tab, m->S, (const unsigned*)seen_stamp, m->slots, base);
    }
    if (rt::stream_sync(h->s0) || rt::check_launch()) return fail(ORBX_E_DEVICE, "local map build failed: %s", rt::last_error());
    for (int b = 0; b < B; b++) { m->sets[b].M = Mb[b]; M_out[b] = Mb[b]; }
    return ORBX_OK;
}

int orbm_map_select(orbx_extractor* h, orbm_map* m, int b, int n, const int* slots) {
    if (int rc = map_call_check(h, m)) return rc;
    if (b < 0 || b >= m->max_sets) return fail(ORBX_E_ARG, "set %d: the map has %d sets", b, m->max_sets);
    if (n < 0 || (n > 0 && !slots)) return fail(ORBX_E_ARG, "set %d: null / negative number of points", b);
    if (n > (1 << 26)) return fail(ORBX_E_CAPACITY, "set %d: at most 2^26 points in a list", b);
    std::lock_guard<std::mutex> lk(m->mu);
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= m->slots) return fail(ORBX_E_ARG, "set %d: slot %d (entry %d) is outside the map's %d slots", b, slots[i], i, m->slots);
        if (!(m->state[slots[i]] & kMapPresent)) return fail(ORBX_E_ARG, "set %d: slot %d (entry %d) holds no point", b, slots[i], i);
    }
    rt::set_device(h->device);
    if (int rc = map_lay_set(m, b, n)) return rc;
    if (n == 0) return ORBX_OK;
    const size_t o_rec = al16(4 * (size_t)n);
    if (int rc = map_stage(m, o_rec + sizeof(MapSetRec), sizeof(MapSetRec))) return rc;
    uint8_t* hp = m->h_stage.p;
    memcpy(hp, slots, 4 * (size_t)n); memcpy(hp + o_rec, &m->set_rec[b], sizeof(MapSetRec));
    if (rt::copy_h2d(m->set_rec[b].slots, hp, 4 * (size_t)n, h->s0) || rt::copy_h2d(m->d_stage.p, hp + o_rec, sizeof(MapSetRec), h->s0)) return fail(ORBX_E_DEVICE, "upload failed: %s", rt::last_error());
    const dim3 grid((unsigned)((4 * (size_t)n + 255) / 256), 1, 1), blk(256, 1, 1);
    ORBX_LAUNCH(k_map_gather, grid, blk, 0, h->s0, (const MapSetRec*)m->d_stage.p, m->S, (const unsigned*)nullptr, m->slots, 0u);
    if (rt::stream_sync(h->s0) || rt::check_launch()) return fail(ORBX_E_DEVICE, "set %d: gather failed: %s", b, rt::last_error());
    m->sets[b].M = n;
    return ORBX_OK;
}

const orbm_points* orbm_map_set(orbx_extractor* h, const orbm_map* m, int b) {
    if (map_call_check(h, m)) return nullptr;
    std::lock_guard<std::mutex> lk(m->mu);
    if (b < 0 || b >= m->max_sets || !m->built[b]) { fail(ORBX_E_ARG, "set %d has not been built (the map has %d sets)", b, m->max_sets); return nullptr; }
    return &m->sets[b];
}

int orbm_map_set_fetch(orbx_extractor* h, const orbm_map* m, int b, int* slots, uint8_t* seen) {
    if (int rc = map_call_check(h, m)) return rc;
    std::lock_guard<std::mutex> lk(m->mu);
    if (b < 0 || b >= m->max_sets || !m->built[b]) return fail(ORBX_E_ARG, "set %d has not been built (the map has %d sets)", b, m->max_sets);
    rt::set_device(h->device);
    const size_t M = m->sets[b].M;
    if (M == 0) return ORBX_OK;
    // the slots and the flags lie side by side in the set's block: one copy brings both
    const uint8_t* src = (const uint8_t*)m->set_rec[b].slots; const size_t o_seen = (size_t)(m->set_rec[b].seen - src), bytes = o_seen + M;
    const uint8_t* got = src;
    if (rt::memory_is_host()) { if (rt::stream_sync(h->s0)) return fail(ORBX_E_DEVICE, "set %d: download failed: %s", b, rt::last_error()); }
    else {
        if (h->h_res.ensure(bytes + 64) || rt::copy_d2h(h->h_res.p, src, bytes, h->s0) || rt::stream_sync(h->s0)) return fail(ORBX_E_DEVICE, "set %d: download failed: %s", b, rt::last_error());
        got = h->h_res.p;
    }
    if (slots) memcpy(slots, got, 4 * M);
    if (seen) memcpy(seen, got + o_seen, M);
    return ORBX_OK;
}

int orbm_points_fetch(orbx_extractor* h, const orbm_points* p, float* pos, float* normal, float* min_distance, float* max_distance, uint8_t* desc) {
    if (!h || !p) return fail(ORBX_E_ARG, "null");
    if (p->device != h->device) return fail(ORBX_E_ARG, "map points live on another device");
    rt::set_device(h->device);
    const size_t M = p->M;
    if (M == 0) return ORBX_OK;
    if ((pos && fetch_sync(h, pos, p->pos, 12 * M)) || (normal && fetch_sync(h, normal, p->normal, 12 * M)) || (min_distance && fetch_sync(h, min_distance, p->min_d, 4 * M)) ||
        (max_distance && fetch_sync(h, max_distance, p->max_d, 4 * M)) || (desc && fetch_sync(h, desc, p->desc, 32 * M)))
        return fail(ORBX_E_DEVICE, "download failed: %s", rt::last_error());
    return ORBX_OK;
}

// MapPoint::ComputeDistinctiveDescriptors on observations that are rows of resident key frames, the winner written into the map's store.  One upload
// (key-frame table | obs_kf | obs_feat | point records), one launch per form that has points (k_distinctive_resident: <= 64 observations in registers,
// more through the LDS), one download of best | best_desc.  Everything is checked before anything is enqueued.
int orbm_distinctive_descriptors_resident(orbx_extractor* h, int nkf, orbm_keyframe* const* kfs, int P, const int* obs_start, const int* obs_kf, const int* obs_feat,
                                          orbm_map* map, const int* slots, int* best, uint8_t* best_desc) {
    if (!h || nkf < 0 || P < 0) return fail(ORBX_E_ARG, "null handle / negative number of key frames or points");
    if (map && map->device != h->device) return fail(ORBX_E_ARG, "the map lives on device %d, the handle on device %d", map->device, h->device);
    if (P == 0) return ORBX_OK;
    if (!obs_start || !best) return fail(ORBX_E_ARG, "null obs_start / best");
    for (int p = 0; p < P; p++) {
        if (obs_start[p] < 0 || obs_start[p + 1] < obs_start[p]) return fail(ORBX_E_ARG, "point %d: obs_start[] must be non-negative and non-decreasing", p);
        if (obs_start[p + 1] - obs_start[p] > kDistinctiveMax)
            return fail(ORBX_E_CAPACITY, "point %d: %d observations, a point may have %d", p, obs_start[p + 1] - obs_start[p], kDistinctiveMax);
    }
    const int o0 = obs_start[0], total = obs_start[P] - o0;
    if (total > 0 && (!kfs || !obs_kf || !obs_feat)) return fail(ORBX_E_ARG, "null key-frame or observation table");
    for (int p = 0; p < P; p++)
        for (int o = obs_start[p]; o < obs_start[p + 1]; o++) {
            const int k = obs_kf[o];
            if (k < 0 || k >= nkf) return fail(ORBX_E_ARG, "observation %d (point %d): key frame %d is outside the call's %d key frames", o, p, k, nkf);
            const orbm_keyframe* kf = kfs[k];
            if (!kf) return fail(ORBX_E_ARG, "observation %d (point %d): key frame %d is null", o, p, k);
            if (kf->device != h->device) return fail(ORBX_E_ARG, "observation %d (point %d): key frame %d lives on device %d, the handle on device %d", o, p, k, kf->device, h->device);
            if (obs_feat[o] < 0 || obs_feat[o] >= kf->N) return fail(ORBX_E_ARG, "observation %d (point %d): feature %d is outside the %d features of key frame %d", o, p, obs_feat[o], kf->N, k);
        }
    const bool writes = map && slots;
    std::unique_lock<std::mutex> lk;
    if (map) lk = std::unique_lock<std::mutex>(map->mu);
    if (writes) {                                                    // slots inside the map, holding a point, each once (-1: the point writes nothing)
        int rc = ORBX_OK, p = 0;
        for (; p < P && !rc; p++) {
            const int s = slots[p];
            if (s == -1) continue;
            if (s < 0 || s >= map->slots) rc = fail(ORBX_E_ARG, "point %d: slot %d is outside the map's %d slots", p, s, map->slots);
            else if (!(map->state[s] & kMapPresent)) rc = fail(ORBX_E_ARG, "point %d: slot %d holds no point", p, s);
            else if (map->mark[s]) rc = fail(ORBX_E_ARG, "point %d: slot %d is written twice in this call", p, s);
            else map->mark[s] = 1;
        }
        for (int q = 0; q < p; q++) if (slots[q] >= 0 && slots[q] < map->slots) map->mark[slots[q]] = 0;
        if (rc) return rc;
    }
    // the launch lists: the points of the register form, then those of the LDS form; a point without observations is in neither (best = -1, :473)
    std::vector<DistinctiveRec> recs; std::vector<int> point_of;
    recs.reserve(P); point_of.reserve(P);
    int largest = 0, n_reg = 0;
    for (int form = 0; form < 2; form++) {
        for (int p = 0; p < P; p++) {
            const int n = obs_start[p + 1] - obs_start[p];
            if (n == 0 || (n > kDistinctiveRegMax) != (form == 1)) continue;
            recs.push_back({writes && slots[p] >= 0 ? map->S.desc + 4 * (size_t)slots[p] : nullptr, obs_start[p] - o0, n});
            point_of.push_back(p);
            largest = std::max(largest, n);
        }
        if (form == 0) n_reg = (int)recs.size();
    }
    for (int p = 0; p < P; p++) best[p] = -1;
    const int n_rec = (int)recs.size(), n_lds = n_rec - n_reg;
    if (n_rec == 0) return ORBX_OK;
    rt::set_device(h->device);
    std::vector<const unsigned long long*> table(nkf);
    for (int k = 0; k < nkf; k++) table[k] = kfs[k] ? kfs[k]->dev.desc : nullptr;
    Packer pk(h);
    const size_t pt = pk.add(table.data(), sizeof(table[0]) * table.size()), pok = pk.add(obs_kf + o0, sizeof(int) * (size_t)total),
                 pof = pk.add(obs_feat + o0, sizeof(int) * (size_t)total), pr = pk.add(recs.data(), sizeof(DistinctiveRec) * recs.size()),
                 pout = pk.room((4 + 32) * (size_t)n_rec);                      // best_desc [n_rec][4], then best [n_rec]
    if (int e = pk.flush()) return fail(ORBX_E_DEVICE, "%s", upload_error(e));
    unsigned long long* d_desc = pk.out<unsigned long long>(pout); int* d_best = (int*)(d_desc + 4 * (size_t)n_rec);
    const DistinctiveRec* d_recs = pk.dev<DistinctiveRec>(pr);
    const unsigned long long* const* d_table = pk.dev<const unsigned long long*>(pt);
    if (n_reg > 0) {
        const dim3 grid((n_reg + 3) / 4, 1, 1), blk(256, 1, 1);
        ORBX_LAUNCH(k_distinctive_resident<false>, grid, blk, 0, h->s0, d_recs, 0, n_reg, d_table, pk.dev<int>(pok), pk.dev<int>(pof), d_best, d_desc);
    }
    if (n_lds > 0) {
        const dim3 grid(n_lds, 1, 1), blk(64, 1, 1);
        ORBX_LAUNCH(k_distinctive_resident<true>, grid, blk, 32 * (size_t)largest, h->s0, d_recs, n_reg, n_lds, d_table, pk.dev<int>(pok), pk.dev<int>(pof), d_best, d_desc);
    }
    const size_t o_best = 32 * (size_t)n_rec, bytes = o_best + 4 * (size_t)n_rec;
    const uint8_t* res = (const uint8_t*)d_desc;
    int e = 0;
    if (!rt::memory_is_host()) {                                                // (without best_desc only the indices come down)
        const size_t from = best_desc ? 0 : o_best;
        e = h->h_res.ensure(bytes + 64);
        if (!e) e = rt::copy_d2h(h->h_res.p + from, res + from, bytes - from, h->s0);
        res = h->h_res.p;
    }
    if (e || rt::stream_sync(h->s0) || rt::check_launch()) return fail(ORBX_E_DEVICE, "distinctive-descriptor kernel failed: %s", rt::last_error());
    const int* got = (const int*)(res + o_best);
    for (int r = 0; r < n_rec; r++) {
        best[point_of[r]] = got[r];
        if (best_desc) memcpy(best_desc + 32 * (size_t)point_of[r], res + 32 * (size_t)r, 32);
    }
    return ORBX_OK;
}

}  // extern "C"

// ---- the tracking searches that name their points by slot or by key-frame row of an orbm_map (include/orbx.h) ----
// Each checks everything it can refuse, takes the map's mutex, and runs the host-fed call's own code with rows that k_map_rows_gather / k_map_row_flags
// write on the device.
namespace {
int map_search_check(const orbx_extractor* h, const orbm_map* m) {
    if (h->device != m->device) return fail(ORBX_E_ARG, "the map lives on device %d, the handle on device %d", m->device, h->device);
    return ORBX_OK;
}
// LastFrame.mvpMapPoints as slots: n[b] rows of frame b are used, each -1 or a slot of the map (whether it holds a point is the device's to read)
int last_slots_check(const orbm_map* m, int B, const OrbmLastFrameSlots* last) {
    if (last->cap_last <= 0 || !last->n || !last->slots || !last->octave || !last->angle) return fail(ORBX_E_ARG, "bad last-frame batch (cap_last, n, slots, octave and angle are required)");
    for (int b = 0; b < B; b++) {
        if (last->n[b] < 0 || last->n[b] > last->cap_last) return fail(ORBX_E_ARG, "frame %d: %d points in %d rows", b, last->n[b], last->cap_last);
        const int* s = last->slots + (size_t)b * last->cap_last;
        for (int i = 0; i < last->n[b]; i++)
            if (s[i] < -1 || s[i] >= m->slots) return fail(ORBX_E_ARG, "frame %d, entry %d: slot %d is outside the map's %d slots", b, i, s[i], m->slots);
    }
    return ORBX_OK;
}
PointRows last_slot_rows(const OrbmLastFrameSlots* last) { return {last->cap_last, last->n, nullptr, nullptr, last->octave, last->angle, last->has_obs, nullptr, nullptr, nullptr}; }
// the key frame of frame b by its row: set, and as long as the resident key frame it is paired with; *n = its length
int map_row_check(const orbx_extractor* h, const orbm_map* m, int b, int row, const orbm_keyframe* K, int* n) {
    if (row < 0 || row >= m->kf_rows) return fail(ORBX_E_ARG, "frame %d: row %d is outside the map's %d key-frame rows", b, row, m->kf_rows);
    if (!m->kf_set[row]) return fail(ORBX_E_ARG, "frame %d: row %d was never set (orbm_map_set_keyframe)", b, row);
    if (!K) return fail(ORBX_E_ARG, "frame %d: null key frame", b);
    if (K->device != h->device) return fail(ORBX_E_ARG, "frame %d: the key frame lives on another device", b);
    if (K->N != m->kf_n[row]) return fail(ORBX_E_ARG, "frame %d: row %d holds %d entries, its key frame %d features", b, row, m->kf_n[row], K->N);
    *n = K->N;
    return ORBX_OK;
}
// the call-time flags of a resident search from checked rows of the map: at most two lists of rows, as CallFlags takes the caller's arrays
CallFlags map_flags(const orbm_map* m, const int* rows0, const int* rows1) { return CallFlags(m->d_kf.p, m->kf_row_cap, m->S.state, rows0, rows1); }
}  // namespace

extern "C" {

int orbm_search_by_projection_lastframe_batch_map(orbx_extractor* h, int first, int B, const OrbmFrustumView* cur, orbm_map* map, const OrbmLastFrameSlots* last, float th,
                                                  const uint8_t* forward, const uint8_t* backward, int check_ori, const uint8_t* occupied, int use_u_right) {
    batch_clear(h);
    if (!h || !cur || !map || !last || B <= 0 || first < 0 || first + B > h->lastB) return fail(ORBX_E_ARG, "bad frame range / null");
    if (int rc = map_search_check(h, map)) return rc;
    if (int rc = last_slots_check(map, B, last)) return rc;
    std::lock_guard<std::mutex> lk(map->mu);
    const MapRows src = {map->S, last->slots, nullptr, last->outlier, (size_t)last->cap_last};
    const PointRows R = last_slot_rows(last);
    return projection_batch(h, first, B, cur, &R, th, forward, backward, check_ori, occupied, use_u_right, false, TH_HIGH, &src);
}

int orbm_search_by_projection_lastframe_rig_batch_map(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const OrbmFrustumRigView* cur, const float* trl,
                                                      orbm_map* map, const OrbmLastFrameSlots* last, float th, const uint8_t* forward, const uint8_t* backward,
                                                      int check_ori, const uint8_t* occupied) {
    batch_clear(L);
    if (!L || !R || !cur || !trl || !map || !last || B <= 0) return fail(ORBX_E_ARG, "null");
    if (int rc = map_search_check(L, map)) return rc;
    if (int rc = last_slots_check(map, B, last)) return rc;
    std::lock_guard<std::mutex> lk(map->mu);
    const MapRows src = {map->S, last->slots, nullptr, last->outlier, (size_t)last->cap_last};
    const PointRows rows = last_slot_rows(last);
    return lastframe_rig_batch(L, lf, R, rf, B, cur, trl, &rows, &src, th, forward, backward, check_ori, occupied);
}

int orbm_search_by_projection_keyframe_batch_map(orbx_extractor* h, int first, int B, const OrbmFrustumView* cur, orbm_map* map, const OrbmKeyFrameRows* kf, float th,
                                                 int orb_dist, int check_ori, const uint8_t* occupied) {
    batch_clear(h);
    if (!h || !cur || !map || !kf || B <= 0 || first < 0 || first + B > h->lastB) return fail(ORBX_E_ARG, "bad frame range / null");
    if (!kf->row || !kf->kfs) return fail(ORBX_E_ARG, "bad key-frame batch (row and kfs are required)");
    if (orb_dist < 0 || orb_dist > 256) return fail(ORBX_E_ARG, "ORBdist out of range");
    if (int rc = map_search_check(h, map)) return rc;
    std::lock_guard<std::mutex> lk(map->mu);
    std::vector<int> n(B); std::vector<MapRowRec> recs(B);
    int M = 1;
    for (int b = 0; b < B; b++) {
        if (int rc = map_row_check(h, map, b, kf->row[b], kf->kfs[b], &n[b])) return rc;
        if (kf->found && kf->cap_found < n[b]) return fail(ORBX_E_ARG, "frame %d: cap_found is %d, row %d holds %d entries", b, kf->cap_found, kf->row[b], n[b]);
        recs[b] = {map->d_kf.p + (size_t)kf->row[b] * map->kf_row_cap, kf->kfs[b]->dev.kps};
        M = std::max(M, n[b]);
    }
    // (has_obs = all, no right-coordinate gate: as orbm_search_by_projection_keyframe_batch)
    const MapRows src = {map->S, nullptr, recs.data(), kf->found, (size_t)(kf->cap_found > 0 ? kf->cap_found : 0)};
    const PointRows R = {M, n.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return projection_batch(h, first, B, cur, &R, th, nullptr, nullptr, check_ori, occupied, /*use_u_right*/ 0, true, orb_dist, &src);
}

int orbm_search_by_bow_frames_batch_map(orbx_extractor* h, const orbv_vocabulary* v, int first, int B, orbm_keyframe* const* KFs, orbm_map* map, const int* rows,
                                        float nnratio, int check_ori, int* const* matches12, int* nmatches_out) {
    if (!h || !v || B <= 0 || !KFs || !map || !rows || !matches12) return fail(ORBX_E_ARG, "null");
    if (int rc = map_search_check(h, map)) return rc;
    const std::unique_lock<std::mutex> vlk = orbv_lock(v);      // the vocabulary's lock first, then the map's mutex (see struct orbm_map)
    std::lock_guard<std::mutex> lk(map->mu);                     // the call is blocking: both are held until the matches are down
    for (int b = 0; b < B; b++) { int n; if (int rc = map_row_check(h, map, b, rows[b], KFs[b], &n)) return rc; }
    return bow_frames_batch_locked(h, v, first, B, KFs, map_flags(map, rows, nullptr), nnratio, check_ori, matches12, nmatches_out);
}

// The three resident searches whose call-time flags are a function of key-frame rows and slot states.  Blocking like their host-fed forms: the map's mutex is
// held until the call returns (the rig BoW form takes the vocabulary's lock first).
static int sft_resident_map(orbx_extractor* h, orbm_keyframe* K1, int row1, int n2, orbm_keyframe* const* K2s, const int* rows2, orbm_map* map, const float* F12s,
                            const OrbmKB8Pair* cams, const float* eps, int only_stereo, int coarse, int check_ori, int* matches12, int* nmatches_out) {
    if (!h || !K1 || !map || n2 < 0 || (n2 > 0 && (!K2s || !rows2 || (!F12s && !cams) || !eps || !matches12))) return fail(ORBX_E_ARG, "null");
    if (int rc = map_search_check(h, map)) return rc;
    std::lock_guard<std::mutex> lk(map->mu);
    int n;
    if (int rc = map_row_check(h, map, 0, row1, K1, &n)) return rc;
    for (int j = 0; j < n2; j++)
        if (int rc = map_row_check(h, map, 1 + j, rows2[j], K2s[j], &n)) return rc;       // ("frame" 1 + j: neighbour j)
    return sft_resident_impl(h, K1, map_flags(map, &row1, rows2), n2, K2s, F12s, cams, eps, only_stereo, coarse, check_ori, matches12, nmatches_out);
}

int orbm_search_for_triangulation_resident_map(orbx_extractor* h, orbm_keyframe* K1, int row1, int n2, orbm_keyframe* const* K2s, const int* rows2, orbm_map* map,
                                               const float* F12s, const float* eps, int only_stereo, int coarse, int check_ori, int* matches12, int* nmatches_out) {
    if (n2 > 0 && !F12s) return fail(ORBX_E_ARG, "null");
    return sft_resident_map(h, K1, row1, n2, K2s, rows2, map, F12s, nullptr, eps, only_stereo, coarse, check_ori, matches12, nmatches_out);
}

int orbm_search_for_triangulation_resident_kb8_map(orbx_extractor* h, orbm_keyframe* K1, int row1, int n2, orbm_keyframe* const* K2s, const int* rows2, orbm_map* map,
                                                   const OrbmKB8Pair* cams, const float* eps, int only_stereo, int coarse, int check_ori, int* matches12,
                                                   int* nmatches_out) {
    if (n2 > 0 && !cams) return fail(ORBX_E_ARG, "null");
    return sft_resident_map(h, K1, row1, n2, K2s, rows2, map, nullptr, cams, eps, only_stereo, coarse, check_ori, matches12, nmatches_out);
}

int orbm_search_by_bow_resident_map(orbx_extractor* h, int n, orbm_keyframe* const* K1s, const int* rows1, orbm_keyframe* const* K2s, const int* rows2, orbm_map* map,
                                    float nnratio, int th_inclusive, int check_ori, int* const* matches12, int* nmatches_out) {
    if (!h || !map || n < 0 || (n > 0 && (!K1s || !rows1 || !K2s || !matches12))) return fail(ORBX_E_ARG, "null");
    if (int rc = map_search_check(h, map)) return rc;
    std::lock_guard<std::mutex> lk(map->mu);
    for (int p = 0; p < n; p++) {
        int m;
        if (int rc = map_row_check(h, map, p, rows1[p], K1s[p], &m)) return rc;
        if (rows2 && rows2[p] != -1) if (int rc = map_row_check(h, map, p, rows2[p], K2s[p], &m)) return rc;
    }
    return bow_resident_impl(h, n, K1s, K2s, map_flags(map, rows1, rows2), nnratio, th_inclusive, check_ori, matches12, nmatches_out);
}

int orbm_search_by_bow_rig_batch_map(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const orbv_vocabulary* v, int P, const int* frame,
                                     orbm_keyframe* const* KFs, orbm_map* map, const int* rows, float nnratio, int check_ori, int* const* assigned, int* nmatches_out) {
    if (!L || !R || !v || B <= 0 || P <= 0 || !frame || !KFs || !map || !rows || !assigned) return fail(ORBX_E_ARG, "null");
    if (int rc = map_search_check(L, map)) return rc;
    const std::unique_lock<std::mutex> vlk = orbv_lock(v);      // the vocabulary's lock first, then the map's mutex (see struct orbm_map)
    std::lock_guard<std::mutex> lk(map->mu);
    for (int p = 0; p < P; p++) { int n; if (int rc = map_row_check(L, map, p, rows[p], KFs[p], &n)) return rc; }
    return bow_rig_batch_locked(L, lf, R, rf, B, v, P, frame, KFs, map_flags(map, rows, nullptr), nnratio, check_ori, assigned, nmatches_out);
}

}  // extern "C"

// ---- LocalMapping's and LoopClosing's batches on a set of the map: exclusions by row or found list, answers in slots, the replay's row changes as one edit ----
// Blocking like their host-fed forms.  The map's mutex is taken first and held until the call returns (so the set cannot be rebuilt under the search), the
// key-frame grid mutex inside fuse_batch_run / sim3_batch_run after it.
namespace {
// the call's range of the map's table by slot: allocated and cleared by the first call that needs it, cleared again only when the epoch is used up
int map_skip_table(orbx_extractor* h, int M, MapSkip* S) {
    orbm_map* m = S->map;
    const size_t bytes = (size_t)m->slots * sizeof(unsigned);
    if (!m->d_table.p) {
        if (m->d_table.ensure((size_t)m->slots) || rt::memset_async(m->d_table.p, 0, bytes, h->s0)) {
            m->d_table.release();
            return fail(ORBX_E_DEVICE, "allocation of the map's table of %d slots failed", m->slots);
        }
        m->tbase = 0;
    } else if ((long long)m->tbase + M > (long long)m->epoch_limit) {
        if (rt::memset_async(m->d_table.p, 0, bytes, h->s0)) return fail(ORBX_E_DEVICE, "clearing the map's table failed: %s", rt::last_error());
        m->tbase = 0;
    }
    S->table = m->d_table.p; S->base = m->tbase; S->top = m->tbase + (unsigned)M;
    m->tbase = S->top;                                              // (whatever happens from here on, what this call leaves in the table is stale for the next one)
    return ORBX_OK;
}
// (caller holds the map's mutex) set `set` as a search takes it
int map_built_set_check(const orbm_map* m, int set) {
    if (set < 0 || set >= m->max_sets || !m->built[set]) return fail(ORBX_E_ARG, "set %d has not been built (the map has %d sets)", set, m->max_sets);
    return ORBX_OK;
}
// (caller holds nothing) both forms of the Fuse batch on a set of the map: want == nullptr the dense one
int fuse_map_run(orbx_extractor* h, int K, const OrbmFuseTarget* targets, const int* rows, const int* feat0, orbm_map* map, int set, float th, int chi2_gate,
                 int* best_idx, int* best_dist, int* kf_slot, const FusePairsWanted* want) {
    if (!h || K < 0) return fail(ORBX_E_ARG, "null / negative number of targets");
    if (!map || !rows) return fail(ORBX_E_ARG, "null map or row list");
    if (int rc = map_search_check(h, map)) return rc;
    if (want) if (int rc = fuse_pairs_check(want->cap, want->start, want->point, want->feat)) return rc;
    std::lock_guard<std::mutex> lk(map->mu);
    if (int rc = map_built_set_check(map, set)) return rc;
    if (K == 0) { if (want) want->start[0] = 0; return ORBX_OK; }
    if (int rc = fuse_targets_check(h, K, targets, chi2_gate)) return rc;
    MapSkip S;
    S.map = map; S.set_slots = map->set_rec[set].slots; S.state = map->S.state; S.kf_slots = map->d_kf.p;
    S.recs.resize(K);
    for (int k = 0; k < K; k++) {
        const int row = rows[k], f0 = feat0 ? feat0[k] : 0, N = targets[k].kf->N;
        if (row < 0 || row >= map->kf_rows) return fail(ORBX_E_ARG, "target %d: row %d is outside the map's %d key-frame rows", k, row, map->kf_rows);
        if (!map->kf_set[row]) return fail(ORBX_E_ARG, "target %d: row %d was never set (orbm_map_set_keyframe)", k, row);
        const int n = map->kf_n[row];
        if (f0 < 0 || (long long)f0 + N > n) return fail(ORBX_E_ARG, "target %d: features [%d, %lld) lie outside row %d of %d entries", k, f0, (long long)f0 + N, row, n);
        S.recs[k] = {(long long)row * map->kf_row_cap, n, f0};
        S.longest = std::max(S.longest, n);
    }
    return fuse_batch_run(h, K, targets, &map->sets[set], nullptr, &S, th, chi2_gate, best_idx, best_dist, kf_slot, want);
}
}  // namespace

extern "C" {

int orbm_fuse_candidates_batch_map(orbx_extractor* h, int K, const OrbmFuseTarget* targets, const int* rows, const int* feat0, orbm_map* map, int set, float th,
                                   int chi2_gate, int* best_idx, int* best_dist, int* kf_slot) {
    return fuse_map_run(h, K, targets, rows, feat0, map, set, th, chi2_gate, best_idx, best_dist, kf_slot, nullptr);
}

int orbm_fuse_pairs_batch_map(orbx_extractor* h, int K, const OrbmFuseTarget* targets, const int* rows, const int* feat0, orbm_map* map, int set, float th,
                              int chi2_gate, int cap, int* start, int* point, int* feat, int* dist, int* point_slot, int* kf_slot) {
    const FusePairsWanted W = {cap, start, point, feat, dist, point_slot, kf_slot};
    return fuse_map_run(h, K, targets, rows, feat0, map, set, th, chi2_gate, nullptr, nullptr, nullptr, &W);
}

int orbm_search_by_projection_sim3_batch_map(orbx_extractor* h, int K, const OrbmSim3Target* targets, orbm_map* map, int set, const int* found_start,
                                             const int* found_slots, float th, float ratio_hamming, int cap, int* assigned, int* nmatches, int* assigned_slot) {
    if (!h || K < 0) return fail(ORBX_E_ARG, "null / negative number of targets");
    if (!map) return fail(ORBX_E_ARG, "null map");
    if (int rc = map_search_check(h, map)) return rc;
    std::lock_guard<std::mutex> lk(map->mu);
    if (int rc = map_built_set_check(map, set)) return rc;
    if (found_start && !found_slots) return fail(ORBX_E_ARG, "found_start without found_slots");
    if (K == 0) return ORBX_OK;
    int n_max = 0;
    if (int rc = sim3_targets_check(h, K, targets, cap, &n_max)) return rc;
    MapSkip S;
    S.map = map; S.set_slots = map->set_rec[set].slots; S.state = map->S.state; S.kf_slots = map->d_kf.p;
    S.recs.assign(K, MapSkipRec{0, 0, 0});
    if (found_start) {
        if (found_start[0] < 0) return fail(ORBX_E_ARG, "target 0: negative found_start");
        for (int k = 0; k < K; k++) {
            if (found_start[k + 1] < found_start[k]) return fail(ORBX_E_ARG, "target %d: found_start decreases", k);
            for (int j = found_start[k]; j < found_start[k + 1]; j++)
                if (found_slots[j] < -1 || found_slots[j] >= map->slots)
                    return fail(ORBX_E_ARG, "target %d, entry %d: found slot %d is outside the map's %d slots", k, j - found_start[k], found_slots[j], map->slots);
            S.recs[k] = {(long long)found_start[k] - found_start[0], found_start[k + 1] - found_start[k], 0};
            S.longest = std::max(S.longest, S.recs[k].n);
        }
        S.found = found_slots + found_start[0]; S.n_found = (size_t)(found_start[K] - found_start[0]);
    }
    return sim3_batch_run(h, K, targets, n_max, &map->sets[set], nullptr, &S, th, ratio_hamming, cap, assigned, nmatches, assigned_slot);
}

int orbm_map_edit_keyframes(orbx_extractor* h, orbm_map* m, int n, const int* row, const int* feat, const int* slot) {
    if (int rc = map_call_check(h, m)) return rc;
    if (n < 0) return fail(ORBX_E_ARG, "negative number of edits");
    if (n == 0) return ORBX_OK;
    if (!row || !feat || !slot) return fail(ORBX_E_ARG, "null");
    if (n > (1 << 26)) return fail(ORBX_E_CAPACITY, "at most 2^26 edits in a call");
    std::lock_guard<std::mutex> lk(m->mu);
    std::vector<std::pair<unsigned long long, int>> keys(n);
    for (int j = 0; j < n; j++) {
        if (row[j] < 0 || row[j] >= m->kf_rows) return fail(ORBX_E_ARG, "edit %d: row %d is outside the map's %d key-frame rows", j, row[j], m->kf_rows);
        if (feat[j] < 0 || feat[j] >= m->kf_n[row[j]]) return fail(ORBX_E_ARG, "edit %d: feature %d is outside row %d of %d entries", j, feat[j], row[j], m->kf_n[row[j]]);
        if (slot[j] < -1 || slot[j] >= m->slots) return fail(ORBX_E_ARG, "edit %d: slot %d is outside the map's %d slots", j, slot[j], m->slots);
        keys[j] = {((unsigned long long)(unsigned)row[j] << 32) | (unsigned)feat[j], j};
    }
    // two edits of one entry: the result would be whichever store comes last
    std::sort(keys.begin(), keys.end());
    for (int j = 1; j < n; j++)
        if (keys[j].first == keys[j - 1].first)
            return fail(ORBX_E_ARG, "edit %d: feature %d of row %d is edited twice (edit %d as well)", keys[j].second, feat[keys[j].second], row[keys[j].second], keys[j - 1].second);
    rt::set_device(h->device);
    const size_t N = n;
    Bump L;
    const size_t o_row = L.take(4 * N), o_feat = L.take(4 * N), o_slot = L.take(4 * N);
    if (int rc = map_stage(m, L.o, L.o)) return rc;
    uint8_t* hp = m->h_stage.p; uint8_t* dp = m->d_stage.p;
    memcpy(hp + o_row, row, 4 * N); memcpy(hp + o_feat, feat, 4 * N); memcpy(hp + o_slot, slot, 4 * N);
    if (rt::copy_h2d(dp, hp, L.o, h->s0)) return fail(ORBX_E_DEVICE, "upload failed: %s", rt::last_error());
    const dim3 grid((unsigned)((N + 255) / 256), 1, 1), blk(256, 1, 1);
    ORBX_LAUNCH(k_map_edit_rows, grid, blk, 0, h->s0, n, (const int*)(dp + o_row), (const int*)(dp + o_feat), (const int*)(dp + o_slot), m->d_kf.p, m->kf_row_cap);
    if (rt::stream_sync(h->s0) || rt::check_launch()) return fail(ORBX_E_DEVICE, "key-frame row edit failed: %s", rt::last_error());
    return ORBX_OK;
}

// The second half of Tracking::CreateNewKeyFrame (src/Tracking.cc:3868-3960) and the loop of Tracking::UpdateLastFrame (:3264-3341) for B frames of the
// last extraction.  Everything that can be refused from the arguments is refused first; then the images' feature counts come down (the `keeps` arrays and
// the rows are that long), the call's table goes up once, k_map_stereo_select sorts, cuts and ranks, its 8 B bytes of counts come down, and only a call
// whose every frame fits its free slots and `cap` reaches k_map_stereo_write.
int orbm_map_stereo_points(orbx_extractor* h, orbm_map* m, int B, const OrbmStereoPointsFrame* frames, const float* cam, float th_depth, int max_points, int mode,
                           int* created, int* processed, int cap, int* feat, int* slot) {
    static const char* const entry = "orbm_map_stereo_points";
    if (int rc = map_call_check(h, m)) return rc;
    if (B < 0 || max_points < 0 || cap < 0) return fail(ORBX_E_ARG, "%s: B, max_points and cap have to be >= 0", entry);
    if (mode != 0 && mode != 1) return fail(ORBX_E_ARG, "%s: mode %d (0 = key-frame points, 1 = temporal points)", entry, mode);
    if (B == 0) return ORBX_OK;
    if (!frames || !cam || !created || !processed || (cap > 0 && (!feat || !slot))) return fail(ORBX_E_ARG, "%s: null argument", entry);
    if (B > 65535) return fail(ORBX_E_CAPACITY, "%s: at most 65535 frames per call", entry);
    if (h->lastB <= 0) return fail(ORBX_E_ARG, "%s: the handle has not extracted anything yet", entry);
    if (undistort_stale(h)) return fail(ORBX_E_ARG, "%s: orbx_set_undistort was called after the last extraction: extract again before making map points of its frames", entry);
    if (h->nlevels < 1 || h->nlevels > kMaxLevels) return fail(ORBX_E_ARG, "%s: bad scale levels", entry);
    size_t nfree_total = 0;
    bool need_n = false;
    for (int b = 0; b < B; b++) {
        const OrbmStereoPointsFrame& F = frames[b];
        if (F.frame < 0 || F.frame >= h->lastB) return fail(ORBX_E_ARG, "%s: frame %d names image %d, the last extraction holds [0, %d)", entry, b, F.frame, h->lastB);
        if (h->ur_B <= 0 || h->ur_gen != h->extract_gen || F.frame < h->ur_first || F.frame >= h->ur_first + h->ur_B || h->depth_is_rig)
            return fail(ORBX_E_ARG, "%s: frame %d: image %d has no depth results of orbm_stereo_match / orbm_stereo_from_depth on this extraction", entry, b, F.frame);
        if (F.nfree < 0 || (F.nfree > 0 && !F.free_slots)) return fail(ORBX_E_ARG, "%s: frame %d: null / negative free slots", entry, b);
        if (F.row < -1 || F.row >= m->kf_rows) return fail(ORBX_E_ARG, "%s: frame %d: row %d is outside the map's %d key-frame rows", entry, b, F.row, m->kf_rows);
        nfree_total += (size_t)F.nfree;
        need_n = need_n || F.keeps || F.row >= 0;
    }
    if (nfree_total > (size_t)0x7fffffff / 8) return fail(ORBX_E_CAPACITY, "%s: %zu free slots in one call", entry, nfree_total);
    std::lock_guard<std::mutex> lk(m->mu);
    {   // a slot twice, a row twice: two frames would write one place
        int rc = ORBX_OK;
        std::vector<int> rows;
        int b = 0, k = 0;
        for (; b < B && !rc; b++) {
            const OrbmStereoPointsFrame& F = frames[b];
            for (k = 0; k < F.nfree; k++) {
                const int s = F.free_slots[k];
                if (s < 0 || s >= m->slots) { rc = fail(ORBX_E_ARG, "%s: frame %d: free slot %d (entry %d) is outside the map's %d slots", entry, b, s, k, m->slots); break; }
                if (m->mark[s]) { rc = fail(ORBX_E_ARG, "%s: frame %d: free slot %d (entry %d) is listed twice in this call", entry, b, s, k); break; }
                m->mark[s] = 1;
            }
            if (rc) break;
            if (F.row >= 0) rows.push_back(F.row);
        }
        for (int bb = 0; bb <= b && bb < B; bb++) {
            const int upto = bb < b ? frames[bb].nfree : k;
            for (int kk = 0; kk < upto; kk++) m->mark[frames[bb].free_slots[kk]] = 0;
        }
        if (rc) return rc;
        std::sort(rows.begin(), rows.end());
        for (size_t r = 1; r < rows.size(); r++)
            if (rows[r] == rows[r - 1]) return fail(ORBX_E_ARG, "%s: row %d is named by two frames", entry, rows[r]);
    }
    rt::set_device(h->device);
    const int kcap = h->kp_total_cap;
    // N of the images: `keeps` is that long, and so is the row a frame writes into
    std::vector<int> nimg((size_t)h->lastB, kcap);
    if (need_n) {
        if (fetch_sync(h, nimg.data(), h->d_nm.p, sizeof(int) * (size_t)h->lastB)) return fail(ORBX_E_DEVICE, "%s: reading the images' feature counts failed: %s", entry, rt::last_error());
        for (int b = 0; b < B; b++) {
            int& n = nimg[frames[b].frame];
            n = std::max(0, std::min(n, kcap));
            if (frames[b].row >= 0 && n > m->kf_row_cap)
                return fail(ORBX_E_ARG, "%s: frame %d: image %d has %d features, the map's rows hold %d", entry, b, frames[b].frame, n, m->kf_row_cap);
        }
    }
    StereoPointsParams P; memset(&P, 0, sizeof P);
    P.cx = cam[0]; P.cy = cam[1]; P.invfx = cam[2]; P.invfy = cam[3]; P.th_depth = th_depth; P.max_points = max_points; P.mode = mode;
    P.nlevels = h->nlevels; P.cap = kcap; P.scale_top = h->scale[h->nlevels - 1];
    for (int l = 0; l < kMaxLevels; l++) P.scale[l] = l < h->nlevels ? h->scale[l] : 1.0f;
    P.sort_cap = 2;
    while (P.sort_cap < kcap && P.sort_cap < kStereoPointsSortMax) P.sort_cap <<= 1;
    while (P.sort_cap > 2 && (size_t)P.sort_cap * 8 + 1024 > rt::lds_limit(h->device)) P.sort_cap >>= 1;      // (a device with less LDS per workgroup than gfx950)
    std::vector<StereoPointsRec> recs(B);
    std::vector<uint8_t> keeps; std::vector<int> fslots; fslots.reserve(nfree_total);
    size_t out_room = 0;
    for (int b = 0; b < B; b++) {
        const OrbmStereoPointsFrame& F = frames[b];
        const size_t f = (size_t)F.frame;
        StereoPointsRec& R = recs[b]; memset(&R, 0, sizeof R);
        R.kps = (h->ex_undist_active ? h->d_kps_un.p : h->d_kps.p) + f * kcap;                      // mvKeysUn
        R.depth = h->d_depth.p + (f - (size_t)h->ur_first) * kcap; R.desc = h->d_desc.p + f * kcap * 4; R.n = h->d_nm.p + f;
        R.keeps_off = -1;
        if (F.keeps) { R.keeps_off = (long long)keeps.size(); keeps.insert(keeps.end(), F.keeps, F.keeps + nimg[f]); }
        R.free_off = (int)fslots.size(); fslots.insert(fslots.end(), F.free_slots, F.free_slots + F.nfree);
        R.row = F.row;
        memcpy(R.Rwc, F.Rwc, sizeof R.Rwc); memcpy(R.Ow, F.Ow, sizeof R.Ow);
        out_room += (size_t)std::min(std::min(F.nfree, cap), kcap);
    }
    Packer pk(h);
    const size_t pr = pk.add(recs.data(), sizeof(StereoPointsRec) * recs.size()), pf = pk.add(fslots.data(), 4 * fslots.size()), pkeep = pk.add(keeps.data(), keeps.size()),
                 pc = pk.room(8 * (size_t)B), pfeat = pk.room(4 * (size_t)B * kcap), pout = pk.room(4 * out_room);
    if (int e = pk.flush()) return fail(ORBX_E_DEVICE, "%s: %s", entry, upload_error(e));
    ORBX_LAUNCH(k_map_stereo_select, dim3(B, 1, 1), dim3(256, 1, 1), 8 * (size_t)P.sort_cap, h->s0, pk.dev<StereoPointsRec>(pr), P, pk.dev<uint8_t>(pkeep), pk.out<int>(pfeat),
                pk.out<int>(pc));
    std::vector<int> cnt(2 * (size_t)B);
    if (fetch_sync(h, cnt.data(), pk.dev<int>(pc), 8 * (size_t)B) || rt::check_launch()) return fail(ORBX_E_DEVICE, "%s: the selection failed: %s", entry, rt::last_error());
    int refused = -1, why = 0, most = 0; size_t total = 0;
    for (int b = 0; b < B; b++) {
        created[b] = cnt[2 * b]; processed[b] = cnt[2 * b + 1];
        if (refused >= 0) continue;
        if (cnt[2 * b] < 0) { refused = b; why = 0; }
        else if (cnt[2 * b] > frames[b].nfree) { refused = b; why = 1; }
        else if (cnt[2 * b] > cap) { refused = b; why = 2; }
        else { most = std::max(most, cnt[2 * b]); total += (size_t)cnt[2 * b]; }
    }
    if (refused >= 0) {
        const int b = refused;
        if (why == 0) return fail(ORBX_E_CAPACITY, "%s: frame %d: %d features with a positive depth, the sort in LDS holds %d", entry, b, processed[b], P.sort_cap);
        if (why == 1) return fail(ORBX_E_CAPACITY, "%s: frame %d creates %d points and was given %d free slots", entry, b, created[b], frames[b].nfree);
        return fail(ORBX_E_CAPACITY, "%s: frame %d creates %d points, cap is %d", entry, b, created[b], cap);
    }
    if (most == 0) return ORBX_OK;
    // a row that is shorter than its image so far (never set, or set for fewer features) reads -1 behind its old end
    for (int b = 0; b < B; b++) {
        const int row = frames[b].row, n = nimg[frames[b].frame];
        if (row >= 0 && m->kf_n[row] < n &&
            rt::memset_async(m->d_kf.p + (size_t)row * m->kf_row_cap + m->kf_n[row], 0xFF, sizeof(int) * (size_t)(n - m->kf_n[row]), h->s0))
            return fail(ORBX_E_DEVICE, "%s: frame %d: clearing the end of row %d failed", entry, b, row);
    }
    ORBX_LAUNCH(k_map_stereo_write, dim3((unsigned)((4 * (size_t)most + 255) / 256), B, 1), dim3(256, 1, 1), 0, h->s0, pk.dev<StereoPointsRec>(pr), P, pk.dev<int>(pf),
                pk.dev<int>(pfeat), pk.dev<int>(pc), m->S, m->d_kf.p, m->kf_row_cap, pk.out<int>(pout));
    std::vector<int> flat(total);
    const int fe = fetch_sync(h, flat.data(), pk.dev<int>(pout), 4 * total) || rt::check_launch();
    // (the launch is behind us either way: the host's picture of the map follows what the kernel was told to write)
    size_t at = 0;
    for (int b = 0; b < B; b++) {
        const OrbmStereoPointsFrame& F = frames[b];
        for (int j = 0; j < created[b]; j++) {
            feat[(size_t)b * cap + j] = flat[at + j]; slot[(size_t)b * cap + j] = F.free_slots[j];
            m->state[F.free_slots[j]] = (uint8_t)kMapPresent;
        }
        at += (size_t)created[b];
        if (F.row >= 0) { m->kf_n[F.row] = std::max(m->kf_n[F.row], nimg[F.frame]); m->kf_set[F.row] = 1; }
    }
    if (fe) return fail(ORBX_E_DEVICE, "%s: writing the points failed: %s", entry, rt::last_error());
    return ORBX_OK;
}

}  // extern "C"

// ---- Tracking::SearchLocalPoints on the map's own sets: frame b against set set0 + b as the last build left it ----
// The set records are copied under the map's mutex; the search then reads the sets' memory from its stream, under the rule every batch on a map's set
// is under: fetch before the set is rebuilt.
namespace {
int map_sets_check(const orbx_extractor* h, const orbm_map* map, int set0, int B, std::vector<MapSetRec>* recs) {
    if (!map) return fail(ORBX_E_ARG, "null map");
    if (int rc = map_search_check(h, map)) return rc;
    if (set0 < 0) return fail(ORBX_E_ARG, "set0 = %d is negative", set0);
    if (B <= 0) return fail(ORBX_E_ARG, "bad frame range");
    if ((long long)set0 + B > map->max_sets) return fail(ORBX_E_CAPACITY, "sets [%d, %lld): the map has %d sets", set0, (long long)set0 + B, map->max_sets);
    std::lock_guard<std::mutex> lk(map->mu);
    recs->assign(map->set_rec.begin() + set0, map->set_rec.begin() + set0 + B);
    for (int b = 0; b < B; b++) (*recs)[b].M = map->built[set0 + b] ? map->sets[set0 + b].M : 0;      // (never built, or its build failed: an empty map)
    return ORBX_OK;
}
}  // namespace

extern "C" {

int orbm_search_local_points_batch_map(orbx_extractor* h, int first, int B, const OrbmFrustumView* frames, orbm_map* map, int set0, const uint8_t* occupied,
                                       int use_u_right, float cos_limit, float th, int far_points, float th_far, float nnratio, int want_in_view) {
    batch_clear(h);
    if (!h || !frames) return fail(ORBX_E_ARG, "null");
    std::vector<MapSetRec> recs;
    if (int rc = map_sets_check(h, map, set0, B, &recs)) return rc;
    return local_points_batch(h, first, B, frames, nullptr, nullptr, nullptr, nullptr, occupied, use_u_right, cos_limit, th, far_points, th_far, nnratio, want_in_view, recs.data());
}

int orbm_search_local_points_rig_batch_map(orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, const OrbmFrustumRigView* frames, orbm_map* map, int set0,
                                           const uint8_t* occupied, float cos_limit, float th, int far_points, float th_far, float nnratio, int want_in_view) {
    batch_clear(L);
    if (!L || !R || !frames) return fail(ORBX_E_ARG, "null");
    std::vector<MapSetRec> recs;
    if (int rc = map_sets_check(L, map, set0, B, &recs)) return rc;
    return local_points_rig_batch(L, lf, R, rf, B, frames, nullptr, nullptr, nullptr, nullptr, occupied, cos_limit, th, far_points, th_far, nnratio, want_in_view, recs.data());
}

int orbm_search_local_points_fetch_slots(orbx_extractor* h, int* assigned_slot, int cap, int* nmatches, uint8_t* in_view) {
    if (!h || h->batch.B <= 0) return fail(ORBX_E_ARG, "no batched local point search is pending");
    if (h->batch.rig) return fail(ORBX_E_ARG, "the pending batch is a rig batch: fetch it with orbm_search_rig_batch_fetch_slots");
    if (!h->batch.slot_result) return fail(ORBX_E_ARG, "the pending batch was not enqueued on a map's sets (orbm_search_local_points_batch_map): it has no slots to return");
    if (assigned_slot && cap < h->kp_total_cap) return fail(ORBX_E_CAPACITY, "assigned rows need %d entries", h->kp_total_cap);
    const bool fetch_view = in_view && h->batch.want_view && h->batch.M > 0;
    const int rc = batch_fetch(h, h->kp_total_cap, "batched local point search", assigned_slot, cap, nmatches, 1, fetch_view, &in_view, true);
    if (rc) return rc;
    if (in_view && !fetch_view) return fail(ORBX_E_ARG, "in_view was not requested at enqueue time");
    return ORBX_OK;
}

int orbm_search_rig_batch_fetch_slots(orbx_extractor* L, int* assigned_slot, int cap, int* nmatches, uint8_t* in_view, uint8_t* in_view_r) {
    if (!L || L->batch.B <= 0 || !L->batch.rig) return fail(ORBX_E_ARG, "no batched rig search is pending");
    if (!L->batch.slot_result) return fail(ORBX_E_ARG, "the pending batch was not enqueued on a map's sets (orbm_search_local_points_rig_batch_map): it has no slots to return");
    if (assigned_slot && cap < 2 * L->kp_total_cap) return fail(ORBX_E_ARG, "assigned rows need %d entries (2 x orbx_max_keypoints)", 2 * L->kp_total_cap);
    if ((in_view || in_view_r) && !L->batch.want_view) return fail(ORBX_E_ARG, "in_view was not requested at enqueue time");
    uint8_t* const views[2] = {in_view, in_view_r};
    return batch_fetch(L, 2 * (size_t)L->kp_total_cap, "batched rig search", assigned_slot, cap, nmatches, 2, L->batch.want_view && L->batch.M > 0, views, true);
}

int orbm_map_sets_fetch(orbx_extractor* h, const orbm_map* m, int set0, int B, const int* start, int* slots, uint8_t* seen) {
    if (int rc = map_call_check(h, m)) return rc;
    if (set0 < 0 || B < 0) return fail(ORBX_E_ARG, "negative set0 / number of sets");
    if (B == 0) return ORBX_OK;
    if (!start) return fail(ORBX_E_ARG, "null start");
    if ((long long)set0 + B > m->max_sets) return fail(ORBX_E_ARG, "sets [%d, %lld): the map has %d sets", set0, (long long)set0 + B, m->max_sets);
    std::lock_guard<std::mutex> lk(m->mu);
    if (start[0] < 0) return fail(ORBX_E_ARG, "set %d: negative start", set0);
    // every set's [slots | .. | seen] lies in one piece of its block: one copy each into the handle's pinned buffer, ONE wait for all of them
    Bump hb;
    std::vector<size_t> at(B);
    for (int b = 0; b < B; b++) {
        const int s = set0 + b;
        if (!m->built[s]) return fail(ORBX_E_ARG, "set %d has not been built (the map has %d sets)", s, m->max_sets);
        const long long span = (long long)start[b + 1] - start[b];
        if (span < (long long)m->sets[s].M) return fail(ORBX_E_ARG, "set %d: its %d entries do not fit the %lld between start[%d] and start[%d]", s, m->sets[s].M, span, b, b + 1);
        const size_t M = m->sets[s].M;
        at[b] = hb.take(M ? (size_t)(m->set_rec[s].seen - (const uint8_t*)m->set_rec[s].slots) + M : 0);
    }
    rt::set_device(h->device);
    const bool direct = rt::memory_is_host();
    if (!direct && h->h_res.ensure(hb.o + 64)) return fail(ORBX_E_DEVICE, "pinned allocation failed");
    for (int b = 0; b < B && !direct; b++) {
        const int s = set0 + b; const size_t M = m->sets[s].M;
        if (!M) continue;
        const uint8_t* src = (const uint8_t*)m->set_rec[s].slots;
        if (rt::copy_d2h(h->h_res.p + at[b], src, (size_t)(m->set_rec[s].seen - src) + M, h->s0)) return fail(ORBX_E_DEVICE, "set %d: download failed: %s", s, rt::last_error());
    }
    if (rt::stream_sync(h->s0)) return fail(ORBX_E_DEVICE, "sets [%d, %d): download failed: %s", set0, set0 + B, rt::last_error());
    for (int b = 0; b < B; b++) {
        const int s = set0 + b; const size_t M = m->sets[s].M;
        if (!M) continue;
        const uint8_t* src = (const uint8_t*)m->set_rec[s].slots; const size_t o_seen = (size_t)(m->set_rec[s].seen - src);
        const uint8_t* got = direct ? src : h->h_res.p + at[b];
        if (slots) memcpy(slots + start[b], got, 4 * M);
        if (seen) memcpy(seen + start[b], got + o_seen, M);
    }
    return ORBX_OK;
}

}  // extern "C"
