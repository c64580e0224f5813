/* KeyFrameDatabase.h — drop-in facade for ORB_SLAM3::KeyFrameDatabase (the reference's include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc):
 * the place-recognition database that Tracking::Relocalization (DetectRelocalizationCandidates) and LoopClosing::NewDetectCommonRegions
 * (DetectNBestCandidates) query, on top of the key frame database of include/orbx.h (orbv_db_*).
 *
 * Division of labour: the inverted-file walk - shared words per key frame, maxCommonWords, minCommonWords = (int)(max * 0.8f), the score of
 * every key frame above it (ScoringObject, bit-exact) and the order in which the walk first meets the key frames - runs on the device for
 * the whole map at once.  The pointer-graph part stays here, on the caller's own objects, in the reference's order: the per-KeyFrame query
 * fields (mnRelocQuery / mnRelocWords / mRelocScore, mnPlaceRecognitionQuery / Words / Score) are written back as the reference writes them,
 * including two quirks later code can see - a key frame already stamped with the current query id is neither reset nor listed and its word
 * counter grows on, and a covisible neighbour stamped by this query but not scored adds its stale score from an earlier query - then the
 * covisibility accumulation, the stable descending sort (DetectNBestCandidates), the 0.75 filter (DetectRelocalizationCandidates) and the
 * map filters.  The key of a key frame on the device is its address.
 *
 * Two divergences, both deliberate: KL scoring is refused when the database is made (its score needs the host's fp64 log), and a bad key
 * frame in the candidate loop of DetectNBestCandidates is skipped - the reference `continue`s there without advancing and spins forever.
 *
 * DetectLoopCandidates, DetectCandidates, DetectBestCandidates, PreSave, PostLoad and SetORBVocabulary have no caller in the reference's
 * src/; they are declared and throw std::runtime_error naming themselves.
 *
 * The methods are templates on the KeyFrame / Frame / Map types (as in ORBmatcher.h): mBowVec is any ascending (word id, value) map, so this
 * header needs neither DBoW2 nor Eigen.  The vocabulary passed to the constructor must expose its device vocabulary as Handle()
 * (ORBVocabularyAmd, include/orb_slam3_amd/ORBVocabulary.h).  Every method holds one mutex, as the reference's do.
 */
#ifndef ORB_SLAM3_AMD_KEYFRAMEDATABASE_H
#define ORB_SLAM3_AMD_KEYFRAMEDATABASE_H
// This header REPLACES the reference's include/KeyFrameDatabase.h and takes its include guard (see ORBextractor.h)
#ifdef KEYFRAMEDATABASE_H
#error "the reference's include/KeyFrameDatabase.h was included before the drop-in KeyFrameDatabase.h: replace that file with this one, or put this directory first on the include path; see INTEGRATION.md section 4d"
#endif
#define KEYFRAMEDATABASE_H

#include <cstdint>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>
#include "ORBmatcher.h"
#include "../orbx.h"

namespace ORB_SLAM3
{

class KeyFrame;
class Frame;
class Map;

class KeyFrameDatabase
{
public:
    template <class VocT>
    explicit KeyFrameDatabase(const VocT& voc) : mpDb(nullptr)
    {
        Check(orbv_db_create(voc.Handle(), ORBmatcher::SharedHandle(), &mpDb));
    }
    ~KeyFrameDatabase() { if (mpDb) orbv_db_destroy(mpDb); }
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

    template <class KeyFrameT>
    void add(KeyFrameT* pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        std::vector<uint32_t> ids; std::vector<double> vals;
        Bow(pKF->mBowVec, ids, vals);
        Check(orbv_db_add(mpDb, Key(pKF), ids.data(), vals.data(), (int)ids.size()));
        Entry& e = mAdds[pKF];
        e.n++;
        e.mapOf = [](void* p) -> const void* { return (const void*)static_cast<KeyFrameT*>(p)->GetMap(); };
    }

    template <class KeyFrameT>
    void erase(KeyFrameT* pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        auto it = mAdds.find(pKF);
        if (it == mAdds.end()) return;
        Check(orbv_db_erase(mpDb, Key(pKF)));
        if (--it->second.n == 0) mAdds.erase(it);
    }

    void clear()
    {
        std::unique_lock<std::mutex> lock(mMutex);
        Check(orbv_db_clear(mpDb));
        mAdds.clear();
    }

    // every entry whose key frame's GetMap() is pMap now
    template <class MapT>
    void clearMap(MapT* pMap)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        std::vector<uint64_t> keys;
        for (auto it = mAdds.begin(); it != mAdds.end();) {
            if (it->second.mapOf(it->first) == (const void*)pMap) { keys.push_back(Key(it->first)); it = mAdds.erase(it); }
            else ++it;
        }
        if (!keys.empty()) Check(orbv_db_erase_keys(mpDb, keys.data(), (int)keys.size()));
    }

    // src/KeyFrameDatabase.cc:827-938
    template <class FrameT, class MapT, class KeyFrameT = KeyFrame>
    std::vector<KeyFrameT*> DetectRelocalizationCandidates(FrameT* F, MapT* pMap)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        Result r;
        Query(F->mBowVec, nullptr, r);
        std::list<KeyFrameT*> lKFsSharingWords;
        std::vector<double> scoreOf(r.keys.size());
        bool repeat = false;
        for (size_t i = 0; i < r.keys.size(); i++) {
            KeyFrameT* pKFi = (KeyFrameT*)(uintptr_t)r.keys[i];
            if (pKFi->mnRelocQuery != F->mnId) { pKFi->mnRelocWords = 0; pKFi->mnRelocQuery = F->mnId; lKFsSharingWords.push_back(pKFi); }
            else repeat = true;
            pKFi->mnRelocWords += r.words[i];
        }
        if (lKFsSharingWords.empty()) return std::vector<KeyFrameT*>();
        int maxCommonWords = 0;
        for (KeyFrameT* k : lKFsSharingWords) if (k->mnRelocWords > maxCommonWords) maxCommonWords = k->mnRelocWords;
        int minCommonWords = maxCommonWords * 0.8f;
        std::map<KeyFrameT*, double> scores;
        Scores<KeyFrameT>(F->mBowVec, nullptr, r, repeat, scores);
        std::list<std::pair<float, KeyFrameT*> > lScoreAndMatch;
        for (KeyFrameT* pKFi : lKFsSharingWords) {
            if (pKFi->mnRelocWords > minCommonWords) {
                float si = (float)scores.at(pKFi);
                pKFi->mRelocScore = si;
                lScoreAndMatch.push_back(std::make_pair(si, pKFi));
            }
        }
        if (lScoreAndMatch.empty()) return std::vector<KeyFrameT*>();
        std::list<std::pair<float, KeyFrameT*> > lAccScoreAndMatch;
        float bestAccScore = 0;
        for (auto it = lScoreAndMatch.begin(); it != lScoreAndMatch.end(); it++) {
            KeyFrameT* pKFi = it->second;
            std::vector<KeyFrameT*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
            float bestScore = it->first;
            float accScore = bestScore;
            KeyFrameT* pBestKF = pKFi;
            for (KeyFrameT* pKF2 : vpNeighs) {
                if (pKF2->mnRelocQuery != F->mnId) continue;
                accScore += pKF2->mRelocScore;
                if (pKF2->mRelocScore > bestScore) { pBestKF = pKF2; bestScore = pKF2->mRelocScore; }
            }
            lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
            if (accScore > bestAccScore) bestAccScore = accScore;
        }
        float minScoreToRetain = 0.75f * bestAccScore;
        std::set<KeyFrameT*> spAlreadyAddedKF;
        std::vector<KeyFrameT*> vpRelocCandidates;
        vpRelocCandidates.reserve(lAccScoreAndMatch.size());
        for (auto it = lAccScoreAndMatch.begin(); it != lAccScoreAndMatch.end(); it++) {
            const float& si = it->first;
            if (si > minScoreToRetain) {
                KeyFrameT* pKFi = it->second;
                if (pKFi->GetMap() != pMap) continue;
                if (!spAlreadyAddedKF.count(pKFi)) { vpRelocCandidates.push_back(pKFi); spAlreadyAddedKF.insert(pKFi); }
            }
        }
        return vpRelocCandidates;
    }

    // src/KeyFrameDatabase.cc:649-825
    template <class KeyFrameT>
    void DetectNBestCandidates(KeyFrameT* pKF, std::vector<KeyFrameT*>& vpLoopCand, std::vector<KeyFrameT*>& vpMergeCand, int nNumCandidates)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        std::set<KeyFrameT*> spConnectedKF = pKF->GetConnectedKeyFrames();
        std::vector<uint64_t> excluded;
        for (KeyFrameT* k : spConnectedKF) excluded.push_back(Key(k));
        Result r;
        Query(pKF->mBowVec, &excluded, r);
        std::list<KeyFrameT*> lKFsSharingWords;
        bool repeat = false;
        for (size_t i = 0; i < r.keys.size(); i++) {
            KeyFrameT* pKFi = (KeyFrameT*)(uintptr_t)r.keys[i];
            if (pKFi->mnPlaceRecognitionQuery != pKF->mnId) { pKFi->mnPlaceRecognitionWords = 0; pKFi->mnPlaceRecognitionQuery = pKF->mnId; lKFsSharingWords.push_back(pKFi); }
            else repeat = true;
            pKFi->mnPlaceRecognitionWords += r.words[i];
        }
        // connected key frames are never stamped: each of their list entries resets the counter and counts one (a single 1 at the end),
        // unless an earlier query with this id stamped them
        for (KeyFrameT* c : spConnectedKF) {
            auto it = mAdds.find(c);
            if (it == mAdds.end()) continue;
            const int shared = SharedWords(pKF->mBowVec, c->mBowVec) * it->second.n;
            if (shared == 0) continue;
            if (c->mnPlaceRecognitionQuery != pKF->mnId) c->mnPlaceRecognitionWords = 1;
            else c->mnPlaceRecognitionWords += shared;
        }
        if (lKFsSharingWords.empty()) return;
        int maxCommonWords = 0;
        for (KeyFrameT* k : lKFsSharingWords) if (k->mnPlaceRecognitionWords > maxCommonWords) maxCommonWords = k->mnPlaceRecognitionWords;
        int minCommonWords = maxCommonWords * 0.8f;
        std::map<KeyFrameT*, double> scores;
        Scores<KeyFrameT>(pKF->mBowVec, &excluded, r, repeat, scores);
        std::list<std::pair<float, KeyFrameT*> > lScoreAndMatch;
        for (KeyFrameT* pKFi : lKFsSharingWords) {
            if (pKFi->mnPlaceRecognitionWords > minCommonWords) {
                float si = (float)scores.at(pKFi);
                pKFi->mPlaceRecognitionScore = si;
                lScoreAndMatch.push_back(std::make_pair(si, pKFi));
            }
        }
        if (lScoreAndMatch.empty()) return;
        std::list<std::pair<float, KeyFrameT*> > lAccScoreAndMatch;
        float bestAccScore = 0;
        for (auto it = lScoreAndMatch.begin(); it != lScoreAndMatch.end(); it++) {
            KeyFrameT* pKFi = it->second;
            std::vector<KeyFrameT*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
            float bestScore = it->first;
            float accScore = bestScore;
            KeyFrameT* pBestKF = pKFi;
            for (KeyFrameT* pKF2 : vpNeighs) {
                if (pKF2->mnPlaceRecognitionQuery != pKF->mnId) continue;
                accScore += pKF2->mPlaceRecognitionScore;
                if (pKF2->mPlaceRecognitionScore > bestScore) { pBestKF = pKF2; bestScore = pKF2->mPlaceRecognitionScore; }
            }
            lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
            if (accScore > bestAccScore) bestAccScore = accScore;
        }
        lAccScoreAndMatch.sort([](const std::pair<float, KeyFrameT*>& a, const std::pair<float, KeyFrameT*>& b) { return a.first > b.first; });
        vpLoopCand.reserve(nNumCandidates);
        vpMergeCand.reserve(nNumCandidates);
        std::set<KeyFrameT*> spAlreadyAddedKF;
        size_t i = 0;
        auto it = lAccScoreAndMatch.begin();
        while (i < lAccScoreAndMatch.size() && ((int)vpLoopCand.size() < nNumCandidates || (int)vpMergeCand.size() < nNumCandidates)) {
            KeyFrameT* pKFi = it->second;
            if (pKFi->isBad()) { i++; it++; continue; }          // the reference does not advance here and spins forever
            if (!spAlreadyAddedKF.count(pKFi)) {
                if (pKF->GetMap() == pKFi->GetMap() && (int)vpLoopCand.size() < nNumCandidates) vpLoopCand.push_back(pKFi);
                else if (pKF->GetMap() != pKFi->GetMap() && (int)vpMergeCand.size() < nNumCandidates && !pKFi->GetMap()->IsBad()) vpMergeCand.push_back(pKFi);
                spAlreadyAddedKF.insert(pKFi);
            }
            i++;
            it++;
        }
    }

    // no caller in the reference's src/
    template <class KeyFrameT> std::vector<KeyFrameT*> DetectLoopCandidates(KeyFrameT*, float) { Unsupported("DetectLoopCandidates"); return {}; }
    template <class KeyFrameT> void DetectCandidates(KeyFrameT*, float, std::vector<KeyFrameT*>&, std::vector<KeyFrameT*>&) { Unsupported("DetectCandidates"); }
    template <class KeyFrameT> void DetectBestCandidates(KeyFrameT*, std::vector<KeyFrameT*>&, std::vector<KeyFrameT*>&, int) { Unsupported("DetectBestCandidates"); }
    void PreSave() { Unsupported("PreSave"); }
    template <class MapIdT> void PostLoad(MapIdT) { Unsupported("PostLoad"); }
    template <class VocT> void SetORBVocabulary(VocT*) { Unsupported("SetORBVocabulary"); }

    orbv_database* Handle() const { return mpDb; }

private:
    struct Entry { int n = 0; const void* (*mapOf)(void*) = nullptr; };
    struct Result { std::vector<uint64_t> keys; std::vector<int> words; std::vector<uint8_t> scored; std::vector<double> score; };

    static void Check(int rc) { if (rc != ORBX_OK) throw std::runtime_error(std::string("KeyFrameDatabase (HIP): ") + orbx_last_error()); }
    static void Unsupported(const char* what) { throw std::runtime_error(std::string("KeyFrameDatabase (HIP): ") + what + " is not supported (the reference's src/ never calls it)"); }
    static uint64_t Key(const void* p) { return (uint64_t)(uintptr_t)p; }
    template <class BowT> static void Bow(const BowT& bow, std::vector<uint32_t>& ids, std::vector<double>& vals)
    {
        ids.clear(); vals.clear();
        for (auto it = bow.begin(); it != bow.end(); ++it) { ids.push_back((uint32_t)it->first); vals.push_back((double)it->second); }
    }
    template <class BowT> static int SharedWords(const BowT& a, const BowT& b)
    {
        int n = 0;
        auto i = a.begin(); auto j = b.begin();
        while (i != a.end() && j != b.end()) { if (i->first == j->first) { n++; ++i; ++j; } else if (i->first < j->first) ++i; else ++j; }
        return n;
    }
    template <class BowT> void Query(const BowT& bow, const std::vector<uint64_t>* excluded, Result& r, int scoreAll = 0)
    {
        std::vector<uint32_t> ids; std::vector<double> vals;
        Bow(bow, ids, vals);
        const int qs[2] = {0, (int)ids.size()};
        const int xs[2] = {0, excluded ? (int)excluded->size() : 0};
        int cap = orbv_db_size(mpDb) > 0 ? orbv_db_size(mpDb) : 1, n = 0, minc = 0;
        r.keys.assign(cap, 0); r.words.assign(cap, 0); r.scored.assign(cap, 0); r.score.assign(cap, 0.0);
        Check(orbv_db_query(mpDb, 1, qs, ids.data(), vals.data(), excluded ? xs : nullptr, excluded && !excluded->empty() ? excluded->data() : nullptr, scoreAll, cap,
                            r.keys.data(), r.words.data(), r.scored.data(), r.score.data(), &n, &minc));
        r.keys.resize(n); r.words.resize(n); r.scored.resize(n); r.score.resize(n);
    }
    // the device scored the keys above its own minCommonWords; with key frames stamped by an earlier query of the same id the host's
    // threshold can differ, and then every sharing key is scored
    template <class KeyFrameT, class BowT>
    void Scores(const BowT& bow, const std::vector<uint64_t>* excluded, const Result& r, bool repeat, std::map<KeyFrameT*, double>& out)
    {
        const Result* src = &r;
        Result all;
        if (repeat) { Query(bow, excluded, all, 1); src = &all; }
        for (size_t i = 0; i < src->keys.size(); i++) if (src->scored[i]) out[(KeyFrameT*)(uintptr_t)src->keys[i]] = src->score[i];
    }

    orbv_database* mpDb;
    std::mutex mMutex;
    std::unordered_map<void*, Entry> mAdds;       // key frames with surviving adds: how many, and how to ask them for their map
};

} // namespace ORB_SLAM3

#endif // ORB_SLAM3_AMD_KEYFRAMEDATABASE_H
