// ref_kfdb_driver.cpp — TEST INFRASTRUCTURE.  The reference's own src/KeyFrameDatabase.cc + include/KeyFrameDatabase.h, compiled unmodified and in place over the
// full world (slam_shim/full_world.h with -DORBX_REFERENCE_KFDB: the reference's KeyFrame, Frame and DBoW2; Map stays the stand-in, with IsBad()), behind a C
// interface that tests/cpp/kfdb_gates_test.cpp loads as the third party beside the facade and the project's restatement: key frames by index, maps by index.
// Key frames are the reference's KeyFrame() objects with the members the database reads set directly (mnId, mBowVec, mpMap, the covisibility lists, the six
// query fields); they live as long as the process.
#include <cstring>
#include <map>
#include <vector>
#include "KeyFrame.h"
#include "Frame.h"
#include "KeyFrameDatabase.h"

using namespace ORB_SLAM3;

namespace {
struct RefWorld {
    ORBVocabulary voc;
    KeyFrameDatabase* db = nullptr;
    Map maps[3];
    std::vector<KeyFrame*> kfs;
    int indexOf(KeyFrame* k) const { for (size_t i = 0; i < kfs.size(); i++) if (kfs[i] == k) return (int)i; return -1; }
};
void set_bow(DBoW2::BowVector& v, int n, const unsigned* ids, const double* vals) { v.clear(); for (int i = 0; i < n; i++) v.insert(v.end(), std::make_pair(ids[i], vals[i])); }
}  // namespace

extern "C" {

void* kr_create(const char* vocabulary_text, int n_keyframes) {
    RefWorld* w = new RefWorld();
    if (!w->voc.loadFromTextFile(vocabulary_text)) { delete w; return nullptr; }
    w->db = new KeyFrameDatabase(w->voc);
    for (int i = 0; i < n_keyframes; i++) w->kfs.push_back(new KeyFrame());
    return w;
}
// everything the database reads of key frame k, as the caller's twin holds it now
void kr_sync(void* wv, int k, unsigned long id, int map, int map_bad, int n_bow, const unsigned* ids, const double* vals, int n_covis, const int* covis, const long* query_fields,
             const float* scores) {
    RefWorld* w = (RefWorld*)wv; KeyFrame* kf = w->kfs[k];
    kf->mnId = id; kf->mpMap = &w->maps[map]; w->maps[map].mbBad = map_bad != 0;
    set_bow(kf->mBowVec, n_bow, ids, vals);
    kf->mvpOrderedConnectedKeyFrames.clear(); kf->mConnectedKeyFrameWeights.clear();
    for (int i = 0; i < n_covis; i++) { kf->mvpOrderedConnectedKeyFrames.push_back(w->kfs[covis[i]]); kf->mConnectedKeyFrameWeights[w->kfs[covis[i]]] = 100 - i; }
    kf->mnRelocQuery = query_fields[0]; kf->mnRelocWords = (int)query_fields[1]; kf->mnPlaceRecognitionQuery = query_fields[2]; kf->mnPlaceRecognitionWords = (int)query_fields[3];
    kf->mRelocScore = scores[0]; kf->mPlaceRecognitionScore = scores[1];
}
void kr_fields(void* wv, int k, long* query_fields, float* scores) {
    KeyFrame* kf = ((RefWorld*)wv)->kfs[k];
    query_fields[0] = (long)kf->mnRelocQuery; query_fields[1] = kf->mnRelocWords; query_fields[2] = (long)kf->mnPlaceRecognitionQuery; query_fields[3] = kf->mnPlaceRecognitionWords;
    scores[0] = kf->mRelocScore; scores[1] = kf->mPlaceRecognitionScore;
}
void kr_add(void* wv, int k) { RefWorld* w = (RefWorld*)wv; w->db->add(w->kfs[k]); }
void kr_erase(void* wv, int k) { RefWorld* w = (RefWorld*)wv; w->db->erase(w->kfs[k]); }
void kr_clear_map(void* wv, int map) { RefWorld* w = (RefWorld*)wv; w->db->clearMap(&w->maps[map]); }
int kr_reloc(void* wv, unsigned long id, int n_bow, const unsigned* ids, const double* vals, int map, int* out, int cap) {
    RefWorld* w = (RefWorld*)wv;
    Frame F; F.mnId = id; set_bow(F.mBowVec, n_bow, ids, vals);
    const std::vector<KeyFrame*> c = w->db->DetectRelocalizationCandidates(&F, &w->maps[map]);
    for (size_t i = 0; i < c.size() && (int)i < cap; i++) out[i] = w->indexOf(c[i]);
    return (int)c.size();
}
void kr_nbest(void* wv, int k, int n, int* loop, int* n_loop, int* merge, int* n_merge, int cap) {
    RefWorld* w = (RefWorld*)wv;
    std::vector<KeyFrame*> l, m;
    w->db->DetectNBestCandidates(w->kfs[k], l, m, n);
    *n_loop = (int)l.size(); *n_merge = (int)m.size();
    for (size_t i = 0; i < l.size() && (int)i < cap; i++) loop[i] = w->indexOf(l[i]);
    for (size_t i = 0; i < m.size() && (int)i < cap; i++) merge[i] = w->indexOf(m[i]);
}

}  // extern "C"
