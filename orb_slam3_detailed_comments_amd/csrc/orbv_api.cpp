// orbv_api.cpp — host side of the vocabulary transform (include/orbx.h "Vocabulary"): flattens an ORBVocabulary
// (DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>, include/ORBVocabulary.h:28-29) into slot arrays whose children are
// contiguous, uploads them once, and runs k_voc_descend + k_voc_assemble (csrc/k_vocab.hip) per batch of descriptors.
// Also the key frame database (include/orbx.h "Key frame database", orbv_db_*): the records live in host vectors in add order and are
// mirrored to the device before a query (the appended tail, or everything after a compaction or growth); k_kfdb_count / _order / _score.
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <unordered_map>
#include "orbx_internal.h"

using namespace orbx;

struct orbv_vocabulary {
    int k = 0, L = 0, scoring = 0, weighting = 0, device = 0;
    int n_nodes = 0;          // without the root
    int n_words = 0;
    int root_children = 0;
    DevBuf<unsigned long long> d_desc; DevBuf<VocSlot> d_slots; DevBuf<double> d_weight;
    // per-call scratch / results (sized by reserve())
    int cap = 0, maxB = 0, lastB = 0, run_cap = 0;      // run_cap: per-image stride of the results of the last run
    int run_first = -1; const void* run_handle = nullptr; uint64_t run_extract_gen = 0;   // orbv_transform_extracted: which images of which extractor the results belong to
    // orbv_transform_rig_extracted: the right handle, its first image and extraction; the frames' rows are in d_fdesc
    bool run_rig = false; int run_first_r = -1; const void* run_handle_r = nullptr; uint64_t run_extract_gen_r = 0;
    DevBuf<unsigned long long> d_fdesc;
    DevBuf<unsigned> d_word, d_node, d_bow_id, d_fv_node, d_fv_feat;
    DevBuf<double> d_wt, d_bow_val;
    DevBuf<int> d_bow_start, d_fv_start, d_nout, d_nfeat;
    // One vocabulary serves the handles - and threads - of its device (Frame::ComputeBoW on Tracking's, KeyFrame::ComputeBoW on LocalMapping's), but it has
    // one scratch and one set of results.  mu: every entry point that touches either holds it for the whole call.  owner: the handle whose run made the
    // results (nullptr: nobody's; orbv_fetch, orbv_db_add_extracted and orbv_db_query_extracted serve no other).  pending: the handle on whose stream a
    // split-protocol run may still be executing (compared, never dereferenced), ev_pending: recorded behind that run's last kernel by the thread that
    // enqueued it - another thread never touches the handle's stream, which may be capturing a graph just then.  A run through another handle makes its
    // own stream wait for the event; a blocking transform ends waited for and records nothing.  orbx_destroy clears both names (orbv_forget_handle).
    mutable std::mutex mu;
    const void* owner = nullptr; const void* pending = nullptr; rt::event_t ev_pending = 0;
};

namespace {

int norm_of(int scoring) {      // ScoringObject.h:74-89: (mustNormalize, norm) of each scoring class
    switch (scoring) { case 0: return 1; case 1: return 2; case 2: case 3: case 4: return 1; default: return 0; }
}

std::mutex& registry_mutex() { static std::mutex m; return m; }
std::vector<orbv_vocabulary*>& registry() { static std::vector<orbv_vocabulary*> r; return r; }

const char* kOverwritten = "the results of this handle's vocabulary transform were overwritten by a later run on the vocabulary: transform again";

// (caller holds v->mu) before a run through h touches the scratch: what another handle's split-protocol run left on its stream comes first.  The scratch may
// also be freed and reallocated by this run (reserve, d_fdesc.ensure): the host waits when it is about to grow.  The same handle again: stream order, no wait.
int order_behind_pending(orbv_vocabulary* v, orbx_extractor* h, bool grows) {
    if (!v->pending || v->pending == (const void*)h) return 0;
    int e = rt::stream_wait_event(h->s0, v->ev_pending);
    if (grows) e |= rt::event_sync(v->ev_pending);
    v->pending = nullptr;
    return e;
}
// fdesc: the rows the run stages in d_fdesc itself (0: it reads an extractor's)
bool scratch_grows(const orbv_vocabulary* v, int cap, int B, size_t fdesc) { return cap > v->cap || B > v->maxB || (fdesc > 0 && (fdesc > v->d_fdesc.n || !v->d_fdesc.p)); }

int reserve(orbv_vocabulary* v, int cap, int B) {
    if (cap <= v->cap && B <= v->maxB) return 0;
    cap = std::max(cap, v->cap); B = std::max(B, v->maxB);
    const size_t t = (size_t)cap * B;
    int e = v->d_word.ensure(t) | v->d_node.ensure(t) | v->d_wt.ensure(t) | v->d_bow_id.ensure(t) | v->d_bow_val.ensure(t) |
            v->d_fv_node.ensure(t) | v->d_fv_feat.ensure(t) | v->d_bow_start.ensure(t + B) | v->d_fv_start.ensure(t + B) |
            v->d_nout.ensure(2 * (size_t)B) | v->d_nfeat.ensure(B);
    if (e) return -1;
    v->cap = cap; v->maxB = B;
    return 0;
}

// the limits of run() on the features per image, checked before anything is enqueued; *P = the key slots k_voc_assemble sorts
int check_capacity(const orbx_extractor* h, int cap, int* P) {
    if (cap > 16384) return fail(ORBX_E_CAPACITY, "more than 16384 features per image");
    *P = 64; while (*P < cap) *P <<= 1;
    // k_voc_assemble sorts one image's (id, feature) keys in LDS: 8 bytes per key slot (+ its static scan scratch)
    if ((size_t)*P * 8 + 1024 > rt::lds_limit(h->device))
        return fail(ORBX_E_CAPACITY, "%d features per image need %zu bytes of LDS for the vocabulary transform, the device allows %zu per workgroup", cap, (size_t)*P * 8 + 1024, rt::lds_limit(h->device));
    return ORBX_OK;
}

// launches the two kernels over B images whose descriptors sit at fdesc[(b*cap + i)*4]; n_feat: device counts or nullptr (n_fixed)
int run(orbv_vocabulary* v, orbx_extractor* h, const unsigned long long* fdesc, const int* n_feat, int n_fixed, int cap, int B, int levelsup) {
    int P = 0;
    if (int rc = check_capacity(h, cap, &P)) return rc;
    v->lastB = 0; v->owner = nullptr;                       // the earlier results are gone from here on, whoever made them
    if (reserve(v, cap, B)) return fail(ORBX_E_DEVICE, "vocabulary scratch allocation failed");
    const long groups = (long)cap * B;
    dim3 g1((unsigned)((groups * 16 + 255) / 256), 1, 1), blk(256, 1, 1);
    ORBX_LAUNCH(k_voc_descend, g1, blk, 0, h->s0, fdesc, n_feat, n_fixed, cap, B, (const unsigned long long*)v->d_desc.p,
                (const VocSlot*)v->d_slots.p, (const double*)v->d_weight.p, v->root_children, v->L - levelsup, v->d_word.p, v->d_node.p, v->d_wt.p);
    dim3 g2((unsigned)B, 1, 1);
    ORBX_LAUNCH(k_voc_assemble, g2, blk, (size_t)P * 8, h->s0, (const unsigned*)v->d_word.p, (const unsigned*)v->d_node.p, (const double*)v->d_wt.p,
                n_feat, n_fixed, cap, P, v->weighting, norm_of(v->scoring), v->d_bow_id.p, v->d_bow_val.p, v->d_bow_start.p, v->d_fv_node.p,
                v->d_fv_start.p, v->d_fv_feat.p, v->d_nout.p);
    if (rt::check_launch()) return fail(ORBX_E_DEVICE, "vocabulary kernels failed to launch: %s", rt::last_error());
    v->lastB = B; v->run_cap = cap; v->run_first = -1; v->run_handle = nullptr; v->owner = h;
    v->run_rig = false; v->run_first_r = -1; v->run_handle_r = nullptr;
    return ORBX_OK;
}

}  // namespace

namespace orbx {
std::unique_lock<std::mutex> orbv_lock(const orbv_vocabulary* v) { return std::unique_lock<std::mutex>(v->mu); }
void orbv_forget_handle(const orbx_extractor* h) {
    std::lock_guard<std::mutex> rk(registry_mutex());
    for (orbv_vocabulary* v : registry()) {
        std::lock_guard<std::mutex> lk(v->mu);
        if (v->pending == (const void*)h) v->pending = nullptr;         // orbx_destroy has waited for the handle's streams
        if (v->owner == (const void*)h) v->owner = nullptr;
    }
}
int orbv_frame_arrays(const orbv_vocabulary* v, VocFrameArrays* out) {
    if (!v || v->lastB <= 0) return -1;
    out->fv_node = (const uint32_t*)v->d_fv_node.p; out->fv_start = v->d_fv_start.p; out->fv_feat = (const int*)v->d_fv_feat.p; out->nout = v->d_nout.p;
    out->cap = v->run_cap; out->lastB = v->lastB; out->device = v->device; out->first = v->run_first; out->handle = v->run_handle; out->extract_gen = v->run_extract_gen;
    out->rig = v->run_rig ? 1 : 0; out->first_r = v->run_first_r; out->handle_r = v->run_handle_r; out->extract_gen_r = v->run_extract_gen_r;
    out->desc = v->run_rig ? (const unsigned long long*)v->d_fdesc.p : nullptr;
    return 0;
}
}  // namespace orbx

extern "C" {

int orbv_create(orbx_extractor* h, int k, int L, int scoring, int weighting, int n_nodes, const int* parent, const uint8_t* is_leaf,
                const uint8_t* desc, const double* weight, orbv_vocabulary** out) {
    if (!h || !out || n_nodes < 0 || (n_nodes > 0 && (!parent || !is_leaf || !desc || !weight))) return fail(ORBX_E_ARG, "null");
    if (scoring < 0 || scoring > 5 || weighting < 0 || weighting > 3) return fail(ORBX_E_ARG, "unknown scoring / weighting type");
    rt::set_device(h->device);
    // node i+1 of the reference = entry i here (loadFromTextFile numbers the nodes by line, TemplatedVocabulary.h:1385-1392); the
    // children of a node keep their line order; word ids are handed out to the nodes flagged as leaves, in line order (:1408-1416)
    std::vector<std::vector<int>> children((size_t)n_nodes + 1);
    for (int i = 0; i < n_nodes; i++) {
        const int p = parent[i];
        if (p < 0 || p > i) return fail(ORBX_E_ARG, "node %d: parent %d must be an earlier node", i + 1, p);
        children[p].push_back(i + 1);
    }
    std::vector<int> word_of((size_t)n_nodes + 1, 0);
    int n_words = 0;
    for (int i = 0; i < n_nodes; i++) if (is_leaf[i]) word_of[i + 1] = n_words++;
    // slots: breadth-first, so that the children of every node are consecutive
    std::vector<int> slot_node; slot_node.reserve(n_nodes);
    std::vector<int> first_child_slot((size_t)n_nodes + 1, 0);
    std::vector<int> queue; queue.push_back(0);
    for (size_t qi = 0; qi < queue.size(); qi++) {
        const int nd = queue[qi];
        first_child_slot[nd] = (int)slot_node.size();
        for (int c : children[nd]) { slot_node.push_back(c); queue.push_back(c); }
    }
    const int ns = (int)slot_node.size();      // == n_nodes (every node hangs below the root)
    std::vector<VocSlot> slots(ns > 0 ? ns : 1);
    std::vector<unsigned long long> sdesc((size_t)(ns > 0 ? ns : 1) * 4);
    std::vector<double> sw(ns > 0 ? ns : 1);
    for (int s = 0; s < ns; s++) {
        const int nd = slot_node[s];
        slots[s].node_id = nd; slots[s].child_start = first_child_slot[nd]; slots[s].child_cnt = (int)children[nd].size();
        slots[s].word_id = word_of[nd];
        if (slots[s].child_cnt > 255) return fail(ORBX_E_ARG, "node %d has more than 255 children", nd);
        memcpy(&sdesc[(size_t)s * 4], desc + 32 * (size_t)(nd - 1), 32);
        sw[s] = weight[nd - 1];
    }
    if (children[0].size() > 255) return fail(ORBX_E_ARG, "the root has more than 255 children");
    orbv_vocabulary* v = new orbv_vocabulary();
    v->k = k; v->L = L; v->scoring = scoring; v->weighting = weighting; v->device = h->device;
    v->n_nodes = n_nodes; v->n_words = n_words; v->root_children = (int)children[0].size();
    int e = v->d_desc.ensure(sdesc.size()) | v->d_slots.ensure(slots.size()) | v->d_weight.ensure(sw.size()) | rt::event_create(&v->ev_pending);
    if (!e) e = rt::copy_h2d(v->d_desc.p, sdesc.data(), sdesc.size() * 8, h->s0) | rt::copy_h2d(v->d_slots.p, slots.data(), slots.size() * sizeof(VocSlot), h->s0) |
                rt::copy_h2d(v->d_weight.p, sw.data(), sw.size() * 8, h->s0) | rt::stream_sync(h->s0);
    if (e) { orbv_destroy(v); return fail(ORBX_E_DEVICE, "vocabulary upload failed"); }
    { std::lock_guard<std::mutex> rk(registry_mutex()); registry().push_back(v); }
    *out = v;
    return ORBX_OK;
}

// ORBvoc.txt: "k L scoring weighting" then one line per node "parent isLeaf d0 .. d31 weight" (TemplatedVocabulary.h:1338-1430)
int orbv_load_text(orbx_extractor* h, const char* path, orbv_vocabulary** out) {
    if (!h || !path || !out) return fail(ORBX_E_ARG, "null");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(ORBX_E_ARG, "cannot open %s", path);
    std::string text;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    fclose(f);
    const char* p = text.c_str();
    char* end = nullptr;
    long hdr[4];
    for (int i = 0; i < 4; i++) { hdr[i] = strtol(p, &end, 10); if (end == p) return fail(ORBX_E_ARG, "bad vocabulary header"); p = end; }
    if (hdr[0] < 0 || hdr[0] > 20 || hdr[1] < 1 || hdr[1] > 10 || hdr[2] < 0 || hdr[2] > 5 || hdr[3] < 0 || hdr[3] > 3)
        return fail(ORBX_E_ARG, "not a vocabulary text file");                       // the reference's own check (:1359)
    std::vector<int> parent; std::vector<uint8_t> leaf, desc; std::vector<double> weight;
    for (;;) {
        while (*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t') p++;
        if (!*p) break;
        long v0 = strtol(p, &end, 10); if (end == p) return fail(ORBX_E_ARG, "bad node line %zu", parent.size() + 1); p = end;
        long v1 = strtol(p, &end, 10); if (end == p) return fail(ORBX_E_ARG, "bad node line %zu", parent.size() + 1); p = end;
        parent.push_back((int)v0); leaf.push_back(v1 > 0 ? 1 : 0);
        for (int i = 0; i < 32; i++) { long d = strtol(p, &end, 10); if (end == p) return fail(ORBX_E_ARG, "bad descriptor in node line %zu", parent.size()); p = end; desc.push_back((uint8_t)d); }
        double w = strtod(p, &end); if (end == p) return fail(ORBX_E_ARG, "bad weight in node line %zu", parent.size()); p = end;
        weight.push_back(w);
    }
    return orbv_create(h, (int)hdr[0], (int)hdr[1], (int)hdr[2], (int)hdr[3], (int)parent.size(), parent.data(), leaf.data(), desc.data(), weight.data(), out);
}

void orbv_destroy(orbv_vocabulary* v) {
    if (!v) return;
    { std::lock_guard<std::mutex> rk(registry_mutex()); auto& r = registry(); r.erase(std::remove(r.begin(), r.end(), v), r.end()); }
    rt::set_device(v->device);
    rt::event_destroy(v->ev_pending);
    v->d_desc.release(); v->d_slots.release(); v->d_weight.release(); v->d_fdesc.release(); v->d_word.release(); v->d_node.release();
    v->d_bow_id.release(); v->d_fv_node.release(); v->d_fv_feat.release(); v->d_wt.release(); v->d_bow_val.release(); v->d_bow_start.release();
    v->d_fv_start.release(); v->d_nout.release(); v->d_nfeat.release();
    delete v;
}

int orbv_words(const orbv_vocabulary* v) { return v ? v->n_words : 0; }

int orbv_transform_extracted(orbv_vocabulary* v, orbx_extractor* h, int first, int B, int levelsup) {
    if (!v || !h) return fail(ORBX_E_ARG, "null");
    if (v->device != h->device) return fail(ORBX_E_ARG, "vocabulary and extractor live on different devices");
    if (first < 0 || B <= 0 || first + B > h->lastB) return fail(ORBX_E_ARG, "images [%d, %d) are not in the last batch of %d", first, first + B, h->lastB);
    rt::set_device(h->device);
    const int cap = h->kp_total_cap;
    std::lock_guard<std::mutex> lk(v->mu);
    if (order_behind_pending(v, h, scratch_grows(v, cap, B, 0))) return fail(ORBX_E_DEVICE, "waiting for the vocabulary's previous run failed: %s", rt::last_error());
    const int rc = run(v, h, (const unsigned long long*)(h->d_desc.p + (size_t)first * cap * 4), (const int*)(h->d_nm.p + first), 0, cap, B, levelsup);
    if (rc == ORBX_OK) { v->run_first = first; v->run_handle = h; v->run_extract_gen = h->extract_gen; rt::event_record(v->ev_pending, h->s0); v->pending = h; }
    return rc;
}

// Frame::ComputeBoW of B rig frames (src/Frame.cc:984-997 over the rig Frame's mDescriptors, :1514): k_voc_gather_rig joins each frame's camera-1 and
// camera-2 rows into d_fdesc, then the transform of orbv_transform_extracted runs on them with 2 x orbx_max_keypoints features per frame.
int orbv_transform_rig_extracted(orbv_vocabulary* v, orbx_extractor* L, int lf, orbx_extractor* R, int rf, int B, int levelsup) {
    if (!v || !L || !R) return fail(ORBX_E_ARG, "null");
    if (B <= 0 || lf < 0 || rf < 0 || lf + B > L->lastB || rf + B > R->lastB)
        return fail(ORBX_E_ARG, "frames [%d, %d) of the left handle / [%d, %d) of the right one are not in their last extractions (%d / %d images)", lf, lf + B, rf, rf + B,
                    L->lastB, R->lastB);
    if (L->kp_total_cap != R->kp_total_cap || L->nlevels != R->nlevels || L->scaleFactor != R->scaleFactor)
        return fail(ORBX_E_ARG, "the two handles differ in orbx_max_keypoints, levels or scale factor");
    if (L->device != R->device || v->device != L->device) return fail(ORBX_E_ARG, "vocabulary and extractors live on different devices");
    rt::set_device(L->device);
    const int cap = L->kp_total_cap, cap2 = 2 * cap;
    int P = 0;
    std::lock_guard<std::mutex> lk(v->mu);
    if (int rc = check_capacity(L, cap2, &P)) return rc;                 // refused before the gather overwrites the rows of an earlier rig run
    if (order_behind_pending(v, L, scratch_grows(v, cap2, B, (size_t)B * cap2 * 4))) return fail(ORBX_E_DEVICE, "waiting for the vocabulary's previous run failed: %s", rt::last_error());
    v->lastB = 0; v->run_rig = false; v->run_handle = nullptr; v->run_handle_r = nullptr; v->owner = nullptr;
    if (v->d_fdesc.ensure((size_t)B * cap2 * 4) || reserve(v, cap2, B)) return fail(ORBX_E_DEVICE, "vocabulary scratch allocation failed");
    if (L != R) { record_done_if_pending(R); rt::stream_wait_event(L->s0, R->ev_done); }          // R's extraction runs on R's stream
    dim3 grid((unsigned)((cap2 + 255) / 256), (unsigned)B, 1), blk(256, 1, 1);
    ORBX_LAUNCH(k_voc_gather_rig, grid, blk, 0, L->s0, (const unsigned long long*)(L->d_desc.p + (size_t)lf * cap * 4), (const int*)(L->d_nm.p + lf),
                (const unsigned long long*)(R->d_desc.p + (size_t)rf * cap * 4), (const int*)(R->d_nm.p + rf), cap, B, v->d_fdesc.p, v->d_nfeat.p);
    const int rc = run(v, L, v->d_fdesc.p, v->d_nfeat.p, 0, cap2, B, levelsup);
    if (rc == ORBX_OK) {
        v->run_first = lf; v->run_handle = L; v->run_extract_gen = L->extract_gen;
        v->run_rig = true; v->run_first_r = rf; v->run_handle_r = R; v->run_extract_gen_r = R->extract_gen;
        rt::event_record(v->ev_pending, L->s0); v->pending = L;
    }
    return rc;
}

}  // extern "C"

namespace {
// (caller holds v->mu) orbv_fetch; h's stream has been waited for when it returns
int fetch_locked(orbv_vocabulary* v, orbx_extractor* h, int b, uint32_t* word_id, uint32_t* node_id, int n_features, uint32_t* bow_id, double* bow_val,
                 int* n_bow, uint32_t* fv_node, int* fv_start, uint32_t* fv_feat, int* n_fv) {
    if (v->lastB > 0 && v->owner != (const void*)h) return fail(ORBX_E_ARG, "%s", kOverwritten);
    if (b < 0 || b >= v->lastB) return fail(ORBX_E_ARG, "image %d is not in the last transformed batch of %d", b, v->lastB);
    rt::set_device(h->device);
    int nout[2] = {0, 0};
    const int cap = v->run_cap;
    const size_t off = (size_t)b * cap, offs = (size_t)b * (cap + 1);
    int e = rt::copy_d2h(nout, v->d_nout.p + 2 * b, sizeof nout, h->s0) | rt::stream_sync(h->s0);
    if (e) return fail(ORBX_E_DEVICE, "vocabulary fetch failed: %s", rt::last_error());
    if (n_features > cap) n_features = cap;
    if (word_id && n_features > 0) e |= rt::copy_d2h(word_id, v->d_word.p + off, 4 * (size_t)n_features, h->s0);
    if (node_id && n_features > 0) e |= rt::copy_d2h(node_id, v->d_node.p + off, 4 * (size_t)n_features, h->s0);
    if (bow_id && nout[0] > 0) e |= rt::copy_d2h(bow_id, v->d_bow_id.p + off, 4 * (size_t)nout[0], h->s0);
    if (bow_val && nout[0] > 0) e |= rt::copy_d2h(bow_val, v->d_bow_val.p + off, 8 * (size_t)nout[0], h->s0);
    if (fv_node && nout[1] > 0) e |= rt::copy_d2h(fv_node, v->d_fv_node.p + off, 4 * (size_t)nout[1], h->s0);
    if (fv_start) e |= rt::copy_d2h(fv_start, v->d_fv_start.p + offs, 4 * (size_t)(nout[1] + 1), h->s0);
    if (fv_feat) {
        int total = 0;
        e |= rt::copy_d2h(&total, v->d_fv_start.p + offs + nout[1], 4, h->s0) | rt::stream_sync(h->s0);
        if (total > 0) e |= rt::copy_d2h(fv_feat, v->d_fv_feat.p + off, 4 * (size_t)total, h->s0);
    }
    e |= rt::stream_sync(h->s0);
    if (e) return fail(ORBX_E_DEVICE, "vocabulary fetch failed: %s", rt::last_error());
    if (n_bow) *n_bow = nout[0];
    if (n_fv) *n_fv = nout[1];
    if (v->pending == (const void*)h) v->pending = nullptr;
    return ORBX_OK;
}
}  // namespace

extern "C" {

int orbv_fetch(orbv_vocabulary* v, orbx_extractor* h, int b, uint32_t* word_id, uint32_t* node_id, int n_features, uint32_t* bow_id, double* bow_val,
               int* n_bow, uint32_t* fv_node, int* fv_start, uint32_t* fv_feat, int* n_fv) {
    if (!v || !h) return fail(ORBX_E_ARG, "null");
    std::lock_guard<std::mutex> lk(v->mu);
    return fetch_locked(v, h, b, word_id, node_id, n_features, bow_id, bow_val, n_bow, fv_node, fv_start, fv_feat, n_fv);
}

int orbv_transform(orbv_vocabulary* v, orbx_extractor* h, const uint8_t* desc, int n, int levelsup, uint32_t* word_id, uint32_t* node_id,
                   uint32_t* bow_id, double* bow_val, int* n_bow, uint32_t* fv_node, int* fv_start, uint32_t* fv_feat, int* n_fv) {
    if (!v || !h || n < 0 || (n > 0 && !desc)) return fail(ORBX_E_ARG, "null");
    if (v->device != h->device) return fail(ORBX_E_ARG, "vocabulary and extractor live on different devices");
    if (n > 16384) return fail(ORBX_E_CAPACITY, "more than 16384 features");
    rt::set_device(h->device);
    const int cap = std::max(n, 1);
    std::lock_guard<std::mutex> lk(v->mu);        // upload, kernels and fetch are one client's: any number of threads may call this on one vocabulary
    if (order_behind_pending(v, h, scratch_grows(v, cap, 1, (size_t)cap * 4))) return fail(ORBX_E_DEVICE, "waiting for the vocabulary's previous run failed: %s", rt::last_error());
    if (v->d_fdesc.ensure((size_t)cap * 4)) return fail(ORBX_E_DEVICE, "allocation failed");
    if (n > 0 && rt::copy_h2d(v->d_fdesc.p, desc, 32 * (size_t)n, h->s0)) return fail(ORBX_E_DEVICE, "upload failed");
    int rc = run(v, h, v->d_fdesc.p, nullptr, n, cap, 1, levelsup); if (rc) return rc;
    return fetch_locked(v, h, 0, word_id, node_id, n, bow_id, bow_val, n_bow, fv_node, fv_start, fv_feat, n_fv);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------------------
// Key frame database
struct orbv_database {
    orbv_vocabulary* voc = nullptr;
    int device = 0, scoring = 0, n_words = 0;
    rt::stream_t s = 0;
    // records in add order: the BowVector of record r is ids / vals [rstart[r], rstart[r] + rn[r])
    std::vector<uint32_t> ids; std::vector<double> vals;
    std::vector<long long> rstart; std::vector<int> rn; std::vector<unsigned long long> rkey; std::vector<uint8_t> rlive;
    struct Key { std::deque<int> recs; int n = 0; uint64_t sum = 0; };   // surviving records of a key, in add order; its vector's size and checksum
    std::unordered_map<unsigned long long, Key> keys;
    long long live = 0, dead_words = 0;
    // device mirror: the arena prefix [0, up_words) and the record tables are current unless dirty
    DevBuf<uint32_t> d_ids; DevBuf<double> d_vals; DevBuf<long long> d_rstart; DevBuf<int> d_rn, d_mult; DevBuf<unsigned long long> d_rkey;
    size_t up_words = 0; bool meta_dirty = true;
    // per-query scratch and results
    DevBuf<uint32_t> d_qid; DevBuf<double> d_qval; DevBuf<int> d_qstart, d_qn, d_xstart, d_xrec, d_cnt, d_first, d_order, d_slist, d_head;
    DevBuf<KfdbHit> d_hits; HostBuf<KfdbHit> h_hits; HostBuf<int> h_head;
};

namespace {

uint64_t bow_checksum(const uint32_t* id, const double* val, int n) {       // FNV-1a over the ids and the bit patterns of the values
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t x) { for (int k = 0; k < 8; k++) { h ^= (x >> (8 * k)) & 0xFFu; h *= 1099511628211ull; } };
    for (int i = 0; i < n; i++) { uint64_t b; memcpy(&b, &val[i], 8); mix(id[i]); mix(b); }
    return h;
}

int db_add_host(orbv_database* db, unsigned long long key, const uint32_t* id, const double* val, int n) {
    for (int i = 0; i < n; i++) {
        if ((int)id[i] >= db->n_words || id[i] >= (uint32_t)db->n_words) return fail(ORBX_E_ARG, "word id %u is not a word of the vocabulary (%d words)", id[i], db->n_words);
        if (i > 0 && id[i] <= id[i - 1]) return fail(ORBX_E_ARG, "BowVector word ids must ascend (entry %d)", i);
    }
    const uint64_t sum = bow_checksum(id, val, n);
    auto it = db->keys.find(key);
    if (it != db->keys.end() && (it->second.n != n || it->second.sum != sum))
        return fail(ORBX_E_ARG, "key %llu was added before with another BowVector (%d words then, %d now)", key, it->second.n, n);
    orbv_database::Key& k = db->keys[key];
    k.n = n; k.sum = sum; k.recs.push_back((int)db->rn.size());
    db->rstart.push_back((long long)db->ids.size()); db->rn.push_back(n); db->rkey.push_back(key); db->rlive.push_back(1);
    db->ids.insert(db->ids.end(), id, id + n); db->vals.insert(db->vals.end(), val, val + n);
    db->live++; db->meta_dirty = true;
    return ORBX_OK;
}

void db_kill(orbv_database* db, int r) { db->rlive[r] = 0; db->live--; db->dead_words += db->rn[r]; db->meta_dirty = true; }

// drops the erased records, keeping the order of the others
void db_compact(orbv_database* db) {
    std::vector<int> remap(db->rn.size(), -1);
    size_t w = 0; int nr = 0;
    for (size_t r = 0; r < db->rn.size(); r++) {
        if (!db->rlive[r]) continue;
        const long long s = db->rstart[r]; const int n = db->rn[r];
        if ((long long)w != s) { memmove(&db->ids[w], &db->ids[s], 4 * (size_t)n); memmove(&db->vals[w], &db->vals[s], 8 * (size_t)n); }
        db->rstart[nr] = (long long)w; db->rn[nr] = n; db->rkey[nr] = db->rkey[r]; db->rlive[nr] = 1;
        remap[r] = nr++; w += n;
    }
    db->ids.resize(w); db->vals.resize(w); db->rstart.resize(nr); db->rn.resize(nr); db->rkey.resize(nr); db->rlive.resize(nr);
    for (auto& kv : db->keys) for (int& r : kv.second.recs) r = remap[r];
    db->dead_words = 0; db->up_words = 0; db->meta_dirty = true;
}

// brings the device mirror up to date: compacts when the arena must grow (or erased words outnumber live ones), uploads the appended tail
// or - after a compaction or growth - everything, and the record tables with the multiplicities (the earliest surviving record of a key
// carries the number of its surviving adds, the others 0)
int db_sync(orbv_database* db) {
    if (!db->meta_dirty && db->up_words == db->ids.size()) return 0;
    const size_t live_words = db->ids.size() - (size_t)db->dead_words;
    if (db->dead_words > 0 && (db->ids.size() > db->d_ids.n || (size_t)db->dead_words > live_words)) db_compact(db);
    const size_t nw = db->ids.size(), R = db->rn.size();
    if (nw > db->d_ids.n) {
        const size_t c = std::max<size_t>(nw + nw / 2, 4096);
        if (db->d_ids.ensure(c) || db->d_vals.ensure(c)) return fail(ORBX_E_DEVICE, "key frame database: arena allocation failed");
        db->up_words = 0;
    }
    if (R > db->d_rn.n) {
        const size_t c = std::max<size_t>(R + R / 2, 256);
        if (db->d_rstart.ensure(c) || db->d_rn.ensure(c) || db->d_mult.ensure(c) || db->d_rkey.ensure(c)) return fail(ORBX_E_DEVICE, "key frame database: allocation failed");
    }
    int e = 0;
    if (nw > db->up_words) {
        e |= rt::copy_h2d(db->d_ids.p + db->up_words, db->ids.data() + db->up_words, 4 * (nw - db->up_words), db->s);
        e |= rt::copy_h2d(db->d_vals.p + db->up_words, db->vals.data() + db->up_words, 8 * (nw - db->up_words), db->s);
    }
    std::vector<int> mult(R, 0);
    for (auto& kv : db->keys) if (!kv.second.recs.empty()) mult[kv.second.recs.front()] = (int)kv.second.recs.size();
    if (R > 0) {
        e |= rt::copy_h2d(db->d_rstart.p, db->rstart.data(), 8 * R, db->s) | rt::copy_h2d(db->d_rn.p, db->rn.data(), 4 * R, db->s) |
             rt::copy_h2d(db->d_mult.p, mult.data(), 4 * R, db->s) | rt::copy_h2d(db->d_rkey.p, db->rkey.data(), 8 * R, db->s);
    }
    // the host vectors are the copies' sources: wait before they can change again
    e |= rt::stream_sync(db->s);
    if (e) return fail(ORBX_E_DEVICE, "key frame database upload failed: %s", rt::last_error());
    db->up_words = nw; db->meta_dirty = false;
    return 0;
}

// the three launches and the copy-back of Q queries whose vectors are described by qs (device pointers); nq_max bounds every query's size
int db_run(orbv_database* db, int Q, KfdbQuerySet qs, int nq_max, const int* x_start, const uint64_t* x_keys, int score_all, int cap,
           uint64_t* keys, int* words, uint8_t* scored, double* score, int* n_out, int* min_common) {
    const int R = (int)db->rn.size();
    // exclusions -> record indices of the keys' earliest surviving records (the only ones that carry a count)
    std::vector<int> xs((size_t)Q + 1, 0), xr;
    if (x_start) {
        for (int q = 0; q < Q; q++) {
            for (int i = x_start[q]; i < x_start[q + 1]; i++) {
                auto it = db->keys.find(x_keys[i]);
                if (it != db->keys.end() && !it->second.recs.empty()) xr.push_back(it->second.recs.front());
            }
            xs[q + 1] = (int)xr.size();
        }
    }
    const size_t lds = rt::lds_limit(db->device);
    if ((size_t)nq_max * 12 + 64 > lds) return fail(ORBX_E_CAPACITY, "a query of %d words needs %zu bytes of LDS, the device allows %zu", nq_max, (size_t)nq_max * 12 + 64, lds);
    int nw = 16;                                               // k_kfdb_order: one row of bin counters per wave
    while (nw > 1 && (size_t)nw * 4 * std::max(nq_max, 1) + 512 > lds) nw--;
    const size_t QR = (size_t)Q * std::max(R, 1);
    int e = db->d_cnt.ensure(QR) | db->d_first.ensure(QR) | db->d_order.ensure(QR) | db->d_slist.ensure(QR) | db->d_hits.ensure(QR) |
            db->d_head.ensure(4 * (size_t)Q) | db->h_head.ensure(4 * (size_t)Q);
    if (x_start) e |= db->d_xstart.ensure((size_t)Q + 1) | db->d_xrec.ensure(std::max<size_t>(xr.size(), 1));
    if (e) return fail(ORBX_E_DEVICE, "key frame database: query scratch allocation failed");
    if (x_start) {
        e |= rt::copy_h2d(db->d_xstart.p, xs.data(), 4 * ((size_t)Q + 1), db->s);
        if (!xr.empty()) e |= rt::copy_h2d(db->d_xrec.p, xr.data(), 4 * xr.size(), db->s);
    }
    if (R > 0) {
        dim3 blk(256, 1, 1), g1((unsigned)((R + kKfdbRecsPerBlock - 1) / kKfdbRecsPerBlock), (unsigned)Q, 1);
        ORBX_LAUNCH(k_kfdb_count, g1, blk, (size_t)nq_max * 4, db->s, (const unsigned*)db->d_ids.p, (const long long*)db->d_rstart.p, (const int*)db->d_rn.p,
                    (const int*)db->d_mult.p, R, qs, db->d_cnt.p, db->d_first.p);
    }
    dim3 g2((unsigned)Q, 1, 1), blk2((unsigned)(64 * nw), 1, 1);
    ORBX_LAUNCH(k_kfdb_order, g2, blk2, (size_t)nw * 4 * std::max(nq_max, 1), db->s, db->d_cnt.p, (const int*)db->d_first.p,
                (const unsigned long long*)db->d_rkey.p, R, qs.n, qs.n_step, x_start ? (const int*)db->d_xstart.p : (const int*)nullptr,
                (const int*)db->d_xrec.p, score_all, db->d_order.p, db->d_hits.p, db->d_slist.p, db->d_head.p);
    if (R > 0) {
        dim3 g3((unsigned)std::min(64, (R + 3) / 4), (unsigned)Q, 1), blk(256, 1, 1);
        ORBX_LAUNCH(k_kfdb_score, g3, blk, (size_t)nq_max * 12, db->s, (const unsigned*)db->d_ids.p, (const double*)db->d_vals.p, (const long long*)db->d_rstart.p,
                    (const int*)db->d_rn.p, qs, (const int*)db->d_order.p, (const int*)db->d_slist.p, (const int*)db->d_head.p, db->d_hits.p, R, db->scoring);
    }
    if (rt::check_launch()) return fail(ORBX_E_DEVICE, "key frame database kernels failed to launch: %s", rt::last_error());
    e = rt::copy_d2h(db->h_head.p, db->d_head.p, 16 * (size_t)Q, db->s) | rt::stream_sync(db->s);
    if (e) return fail(ORBX_E_DEVICE, "key frame database query failed: %s", rt::last_error());
    int too_small = 0;
    size_t total = 0;
    for (int q = 0; q < Q; q++) {
        const int n = db->h_head.p[4 * q];
        if (n_out) n_out[q] = n;
        if (min_common) min_common[q] = db->h_head.p[4 * q + 1];
        if (n > cap) too_small = 1;
        total += (size_t)n;
    }
    if (too_small) return fail(ORBX_E_CAPACITY, "a query shares words with more keys than cap = %d (n_out holds the sizes needed)", cap);
    if (db->h_hits.ensure(std::max<size_t>(total, 1))) return fail(ORBX_E_DEVICE, "key frame database: staging allocation failed");
    size_t o = 0;
    for (int q = 0; q < Q; q++) {
        const int n = db->h_head.p[4 * q];
        if (n > 0) e |= rt::copy_d2h(db->h_hits.p + o, db->d_hits.p + (size_t)q * R, sizeof(KfdbHit) * (size_t)n, db->s);
        o += (size_t)n;
    }
    e |= rt::stream_sync(db->s);
    if (e) return fail(ORBX_E_DEVICE, "key frame database query failed: %s", rt::last_error());
    o = 0;
    for (int q = 0; q < Q; q++) {
        const int n = db->h_head.p[4 * q];
        for (int i = 0; i < n; i++) {
            const KfdbHit& h = db->h_hits.p[o + i];
            const size_t d = (size_t)q * cap + i;
            if (keys) keys[d] = h.key;
            if (words) words[d] = h.words;
            if (scored) scored[d] = (uint8_t)h.scored;
            if (score) score[d] = h.score;
        }
        o += (size_t)n;
    }
    return ORBX_OK;
}

}  // namespace

extern "C" {

int orbv_db_create(orbv_vocabulary* v, orbx_extractor* h, orbv_database** out) {
    if (!v || !h || !out) return fail(ORBX_E_ARG, "null");
    if (v->device != h->device) return fail(ORBX_E_ARG, "vocabulary and extractor live on different devices");
    if (v->scoring == 3) return fail(ORBX_E_ARG, "KL scoring is not supported by the key frame database (its score needs the fp64 log of the host's libm)");
    rt::set_device(v->device);
    orbv_database* db = new orbv_database();
    db->voc = v; db->device = v->device; db->scoring = v->scoring; db->n_words = v->n_words;
    if (rt::stream_create(&db->s)) { delete db; return fail(ORBX_E_DEVICE, "stream creation failed: %s", rt::last_error()); }
    *out = db;
    return ORBX_OK;
}

void orbv_db_destroy(orbv_database* db) {
    if (!db) return;
    rt::set_device(db->device);
    rt::stream_sync(db->s);
    db->d_ids.release(); db->d_vals.release(); db->d_rstart.release(); db->d_rn.release(); db->d_mult.release(); db->d_rkey.release();
    db->d_qid.release(); db->d_qval.release(); db->d_qstart.release(); db->d_qn.release(); db->d_xstart.release(); db->d_xrec.release();
    db->d_cnt.release(); db->d_first.release(); db->d_order.release(); db->d_slist.release(); db->d_head.release(); db->d_hits.release();
    db->h_hits.release(); db->h_head.release();
    rt::stream_destroy(db->s);
    delete db;
}

int orbv_db_add(orbv_database* db, uint64_t key, const uint32_t* bow_id, const double* bow_val, int n) {
    if (!db || n < 0 || (n > 0 && (!bow_id || !bow_val))) return fail(ORBX_E_ARG, "null");
    return db_add_host(db, key, bow_id, bow_val, n);
}

int orbv_db_add_extracted(orbv_database* db, uint64_t key, orbx_extractor* h, int b) {
    if (!db || !h) return fail(ORBX_E_ARG, "null");
    orbv_vocabulary* v = db->voc;
    if (h->device != db->device) return fail(ORBX_E_ARG, "extractor and database live on different devices");
    std::lock_guard<std::mutex> lk(v->mu);
    if (v->lastB > 0 && v->owner != (const void*)h) return fail(ORBX_E_ARG, "%s", kOverwritten);
    if (b < 0 || b >= v->lastB) return fail(ORBX_E_ARG, "image %d is not in the last transformed batch of %d", b, v->lastB);
    rt::set_device(db->device);
    int n = 0;
    if (rt::copy_d2h(&n, v->d_nout.p + 2 * b, sizeof n, h->s0) || rt::stream_sync(h->s0)) return fail(ORBX_E_DEVICE, "fetch failed: %s", rt::last_error());
    std::vector<uint32_t> id(std::max(n, 1)); std::vector<double> val(std::max(n, 1));
    const size_t off = (size_t)b * v->run_cap;
    if (n > 0 && (rt::copy_d2h(id.data(), v->d_bow_id.p + off, 4 * (size_t)n, h->s0) || rt::copy_d2h(val.data(), v->d_bow_val.p + off, 8 * (size_t)n, h->s0) ||
                  rt::stream_sync(h->s0)))
        return fail(ORBX_E_DEVICE, "fetch failed: %s", rt::last_error());
    if (v->pending == (const void*)h) v->pending = nullptr;
    return db_add_host(db, key, id.data(), val.data(), n);
}

int orbv_db_erase(orbv_database* db, uint64_t key) {
    if (!db) return fail(ORBX_E_ARG, "null");
    auto it = db->keys.find(key);
    if (it == db->keys.end()) return ORBX_OK;
    db_kill(db, it->second.recs.front());
    it->second.recs.pop_front();
    if (it->second.recs.empty()) db->keys.erase(it);
    return ORBX_OK;
}

int orbv_db_erase_keys(orbv_database* db, const uint64_t* keys, int n) {
    if (!db || n < 0 || (n > 0 && !keys)) return fail(ORBX_E_ARG, "null");
    for (int i = 0; i < n; i++) {
        auto it = db->keys.find(keys[i]);
        if (it == db->keys.end()) continue;
        for (int r : it->second.recs) db_kill(db, r);
        db->keys.erase(it);
    }
    return ORBX_OK;
}

int orbv_db_clear(orbv_database* db) {
    if (!db) return fail(ORBX_E_ARG, "null");
    db->ids.clear(); db->vals.clear(); db->rstart.clear(); db->rn.clear(); db->rkey.clear(); db->rlive.clear(); db->keys.clear();
    db->live = 0; db->dead_words = 0; db->up_words = 0; db->meta_dirty = true;
    return ORBX_OK;
}

int orbv_db_size(const orbv_database* db) { return db ? (int)db->live : 0; }

int orbv_db_query(orbv_database* db, int Q, const int* q_start, const uint32_t* q_ids, const double* q_vals, const int* x_start, const uint64_t* x_keys,
                  int score_all, int cap, uint64_t* keys, int* words, uint8_t* scored, double* score, int* n_out, int* min_common) {
    if (!db || Q <= 0 || !q_start || cap < 0 || (x_start && !x_keys && x_start[Q] > 0)) return fail(ORBX_E_ARG, "null");
    const int total = q_start[Q];
    if (q_start[0] != 0 || total < 0 || (total > 0 && (!q_ids || !q_vals))) return fail(ORBX_E_ARG, "q_start must run from 0 to the number of words");
    std::vector<int> qn(Q);
    int nq_max = 0;
    for (int q = 0; q < Q; q++) {
        qn[q] = q_start[q + 1] - q_start[q];
        if (qn[q] < 0) return fail(ORBX_E_ARG, "q_start must not descend");
        nq_max = std::max(nq_max, qn[q]);
        for (int i = q_start[q] + 1; i < q_start[q + 1]; i++) if (q_ids[i] <= q_ids[i - 1]) return fail(ORBX_E_ARG, "query %d: word ids must ascend", q);
    }
    if (x_start) for (int q = 0; q < Q; q++) if (x_start[q + 1] < x_start[q] || x_start[0] != 0) return fail(ORBX_E_ARG, "x_start must run from 0 and not descend");
    rt::set_device(db->device);
    if (db_sync(db)) return ORBX_E_DEVICE;
    int e = db->d_qid.ensure(std::max(total, 1)) | db->d_qval.ensure(std::max(total, 1)) | db->d_qstart.ensure((size_t)Q + 1) | db->d_qn.ensure(Q);
    if (e) return fail(ORBX_E_DEVICE, "key frame database: query allocation failed");
    if (total > 0) e |= rt::copy_h2d(db->d_qid.p, q_ids, 4 * (size_t)total, db->s) | rt::copy_h2d(db->d_qval.p, q_vals, 8 * (size_t)total, db->s);
    e |= rt::copy_h2d(db->d_qstart.p, q_start, 4 * ((size_t)Q + 1), db->s) | rt::copy_h2d(db->d_qn.p, qn.data(), 4 * (size_t)Q, db->s);
    if (e) return fail(ORBX_E_DEVICE, "key frame database: query upload failed: %s", rt::last_error());
    KfdbQuerySet qs = {db->d_qid.p, db->d_qval.p, db->d_qstart.p, 0, db->d_qn.p, 1};
    return db_run(db, Q, qs, nq_max, x_start, x_keys, score_all, cap, keys, words, scored, score, n_out, min_common);
}

int orbv_db_query_extracted(orbv_database* db, orbx_extractor* h, int first, int Q, const int* x_start, const uint64_t* x_keys, int score_all, int cap,
                            uint64_t* keys, int* words, uint8_t* scored, double* score, int* n_out, int* min_common) {
    if (!db || !h || Q <= 0 || cap < 0 || (x_start && !x_keys && x_start[Q] > 0)) return fail(ORBX_E_ARG, "null");
    orbv_vocabulary* v = db->voc;
    if (h->device != db->device) return fail(ORBX_E_ARG, "extractor and database live on different devices");
    std::lock_guard<std::mutex> lk(v->mu);         // held until db_run has read the BowVectors where the transform left them
    if (v->lastB > 0 && v->owner != (const void*)h) return fail(ORBX_E_ARG, "%s", kOverwritten);
    if (first < 0 || first + Q > v->lastB) return fail(ORBX_E_ARG, "images [%d, %d) are not in the last transformed batch of %d", first, first + Q, v->lastB);
    if (x_start) for (int q = 0; q < Q; q++) if (x_start[q + 1] < x_start[q] || x_start[0] != 0) return fail(ORBX_E_ARG, "x_start must run from 0 and not descend");
    rt::set_device(db->device);
    if (db_sync(db)) return ORBX_E_DEVICE;
    if (rt::stream_sync(h->s0)) return fail(ORBX_E_DEVICE, "vocabulary transform failed: %s", rt::last_error());   // the BowVectors are written on h's stream
    if (v->pending == (const void*)h) v->pending = nullptr;
    const int cap_v = v->run_cap;
    KfdbQuerySet qs = {v->d_bow_id.p + (size_t)first * cap_v, v->d_bow_val.p + (size_t)first * cap_v, nullptr, cap_v, v->d_nout.p + 2 * first, 2};
    return db_run(db, Q, qs, cap_v, x_start, x_keys, score_all, cap, keys, words, scored, score, n_out, min_common);
}

}  // extern "C"
