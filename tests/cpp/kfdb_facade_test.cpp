// kfdb_facade_test.cpp — drives include/orb_slam3_amd/KeyFrameDatabase.h (on the emulator or the HIP library) and a host restatement of
// KeyFrameDatabase (std::list inverted file, the walk and the candidate selection as src/KeyFrameDatabase.cc describes them, scores from the
// reference's own DBoW2 through ref_voc_score) on twin worlds of mock key frames, and compares the candidate vectors and every key frame's
// query fields after every call.  Last, one database shared by three threads (ThreadedSection).
// argv: vocabulary text file, seed, [bench N Q: time the restatement's DetectRelocalizationCandidates]
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <map>
#include <random>
#include <set>
#include <thread>
#include <vector>
#include "ORBmatcher.h"
#include "KeyFrameDatabase.h"

extern "C" {
void* ref_voc_load_text(const char* path);
double ref_voc_score(void* h, const unsigned* id1, const double* v1, int n1, const unsigned* id2, const double* v2, int n2);
}

typedef std::map<unsigned int, double> Bow;

namespace ORB_SLAM3 {
class Map { public: bool bad = false; bool IsBad() { return bad; } };
class KeyFrame {
public:
    long unsigned int mnId = 0;
    Bow mBowVec;
    long unsigned int mnRelocQuery = 0, mnPlaceRecognitionQuery = 0;
    int mnRelocWords = 0, mnPlaceRecognitionWords = 0;
    float mRelocScore = 0, mPlaceRecognitionScore = 0;
    bool bad = false;
    Map* map = nullptr;
    std::vector<KeyFrame*> covis;           // best first
    std::set<KeyFrame*> GetConnectedKeyFrames() { return std::set<KeyFrame*>(covis.begin(), covis.end()); }
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(int n) { return std::vector<KeyFrame*>(covis.begin(), covis.begin() + std::min<size_t>(n, covis.size())); }
    Map* GetMap() { return map; }
    bool isBad() { return bad; }
};
class Frame { public: long unsigned int mnId = 0; Bow mBowVec; };
}  // namespace ORB_SLAM3
using namespace ORB_SLAM3;

struct Voc {
    orbv_vocabulary* v = nullptr;
    orbv_vocabulary* Handle() const { return v; }
};

static void* g_ref = nullptr;
static double RefScore(const Bow& a, const Bow& b) {
    std::vector<unsigned> ia, ib; std::vector<double> va, vb;
    for (auto& kv : a) { ia.push_back(kv.first); va.push_back(kv.second); }
    for (auto& kv : b) { ib.push_back(kv.first); vb.push_back(kv.second); }
    return ref_voc_score(g_ref, ia.data(), va.data(), (int)ia.size(), ib.data(), vb.data(), (int)ib.size());
}

// the restatement: the reference's data structure and walk, on the twin world
struct RestatedDB {
    std::vector<std::list<KeyFrame*> > inv;
    explicit RestatedDB(int n) : inv(n) {}
    void add(KeyFrame* k) { for (auto& kv : k->mBowVec) inv[kv.first].push_back(k); }
    void erase(KeyFrame* k) {
        for (auto& kv : k->mBowVec) { auto& l = inv[kv.first]; for (auto it = l.begin(); it != l.end(); ++it) if (*it == k) { l.erase(it); break; } }
    }
    void clearMap(Map* m) { for (auto& l : inv) for (auto it = l.begin(); it != l.end();) { if ((*it)->GetMap() == m) it = l.erase(it); else ++it; } }
    std::vector<KeyFrame*> Reloc(Frame* F, Map* pMap) {
        std::list<KeyFrame*> sharing;
        for (auto& kv : F->mBowVec) for (KeyFrame* k : inv[kv.first]) {
            if (k->mnRelocQuery != F->mnId) { k->mnRelocWords = 0; k->mnRelocQuery = F->mnId; sharing.push_back(k); }
            k->mnRelocWords++;
        }
        if (sharing.empty()) return {};
        int mx = 0; for (KeyFrame* k : sharing) mx = std::max(mx, k->mnRelocWords);
        int minc = mx * 0.8f;
        std::list<std::pair<float, KeyFrame*> > sm;
        for (KeyFrame* k : sharing) if (k->mnRelocWords > minc) { float si = (float)RefScore(F->mBowVec, k->mBowVec); k->mRelocScore = si; sm.push_back({si, k}); }
        if (sm.empty()) return {};
        std::list<std::pair<float, KeyFrame*> > acc; float best = 0;
        for (auto& p : sm) {
            float bs = p.first, a = bs; KeyFrame* bk = p.second;
            for (KeyFrame* k2 : p.second->GetBestCovisibilityKeyFrames(10)) {
                if (k2->mnRelocQuery != F->mnId) continue;
                a += k2->mRelocScore; if (k2->mRelocScore > bs) { bk = k2; bs = k2->mRelocScore; }
            }
            acc.push_back({a, bk}); if (a > best) best = a;
        }
        float keep = 0.75f * best; std::set<KeyFrame*> seen; std::vector<KeyFrame*> out;
        for (auto& p : acc) if (p.first > keep && p.second->GetMap() == pMap && !seen.count(p.second)) { out.push_back(p.second); seen.insert(p.second); }
        return out;
    }
    void NBest(KeyFrame* pKF, std::vector<KeyFrame*>& loop, std::vector<KeyFrame*>& merge, int n) {
        std::list<KeyFrame*> sharing; std::set<KeyFrame*> conn = pKF->GetConnectedKeyFrames();
        for (auto& kv : pKF->mBowVec) for (KeyFrame* k : inv[kv.first]) {
            if (k->mnPlaceRecognitionQuery != pKF->mnId) { k->mnPlaceRecognitionWords = 0; if (!conn.count(k)) { k->mnPlaceRecognitionQuery = pKF->mnId; sharing.push_back(k); } }
            k->mnPlaceRecognitionWords++;
        }
        if (sharing.empty()) return;
        int mx = 0; for (KeyFrame* k : sharing) mx = std::max(mx, k->mnPlaceRecognitionWords);
        int minc = mx * 0.8f;
        std::list<std::pair<float, KeyFrame*> > sm;
        for (KeyFrame* k : sharing) if (k->mnPlaceRecognitionWords > minc) { float si = (float)RefScore(pKF->mBowVec, k->mBowVec); k->mPlaceRecognitionScore = si; sm.push_back({si, k}); }
        if (sm.empty()) return;
        std::list<std::pair<float, KeyFrame*> > acc;
        for (auto& p : sm) {
            float bs = p.first, a = bs; KeyFrame* bk = p.second;
            for (KeyFrame* k2 : p.second->GetBestCovisibilityKeyFrames(10)) {
                if (k2->mnPlaceRecognitionQuery != pKF->mnId) continue;
                a += k2->mPlaceRecognitionScore; if (k2->mPlaceRecognitionScore > bs) { bk = k2; bs = k2->mPlaceRecognitionScore; }
            }
            acc.push_back({a, bk});
        }
        acc.sort([](const std::pair<float, KeyFrame*>& a, const std::pair<float, KeyFrame*>& b) { return a.first > b.first; });
        std::set<KeyFrame*> seen;
        for (auto& p : acc) {
            if ((int)loop.size() >= n && (int)merge.size() >= n) break;
            KeyFrame* k = p.second;
            if (k->isBad()) continue;           // (the reference spins here; both sides skip)
            if (!seen.count(k)) {
                if (pKF->GetMap() == k->GetMap() && (int)loop.size() < n) loop.push_back(k);
                else if (pKF->GetMap() != k->GetMap() && (int)merge.size() < n && !k->GetMap()->IsBad()) merge.push_back(k);
                seen.insert(k);
            }
        }
    }
};

struct World {
    std::vector<KeyFrame> kf; Map maps[3];
    void build(std::mt19937& g, int N, int nwords, int nlocal = 40, int nextra = 8) {
        kf.assign(N, KeyFrame());
        std::uniform_real_distribution<double> u(0.05, 1.0);
        for (int i = 0; i < N; i++) {
            kf[i].mnId = 1000 + i;
            const int span = nlocal * 3 / 2, base = (i * (nlocal / 6 + 1)) % std::max(1, nwords - span);
            for (int j = 0; j < nlocal; j++) { unsigned w = (unsigned)(base + g() % span); kf[i].mBowVec[w] = u(g); }
            for (int j = 0; j < nextra; j++) kf[i].mBowVec[(unsigned)(g() % nwords)] = u(g);
            if (i % 10 == 9) kf[i].mBowVec = kf[(g() % i)].mBowVec;       // revisits
            kf[i].map = &maps[i < N * 3 / 4 ? 0 : 1];
        }
        for (int i = 0; i < N; i++) {
            std::set<int> nb;
            for (int d = 1; d <= 6; d++) { if (i - d >= 0) nb.insert(i - d); if (i + d < N) nb.insert(i + d); }
            nb.insert((int)(g() % N)); nb.erase(i);
            std::vector<int> v(nb.begin(), nb.end()); std::shuffle(v.begin(), v.end(), g);
            for (int x : v) kf[i].covis.push_back(&kf[x]);
        }
    }
};

static int g_fail = 0;
static void Same(World& a, World& b, const char* what, int step) {
    for (size_t i = 0; i < a.kf.size(); i++) {
        const KeyFrame &x = a.kf[i], &y = b.kf[i];
        if (x.mnRelocQuery != y.mnRelocQuery || x.mnRelocWords != y.mnRelocWords || x.mRelocScore != y.mRelocScore ||
            x.mnPlaceRecognitionQuery != y.mnPlaceRecognitionQuery || x.mnPlaceRecognitionWords != y.mnPlaceRecognitionWords ||
            x.mPlaceRecognitionScore != y.mPlaceRecognitionScore) {
            if (g_fail++ < 10) printf("FIELDS %s step %d kf %zu: reloc %lu/%lu %d/%d %a/%a pr %lu/%lu %d/%d %a/%a\n", what, step, i, x.mnRelocQuery, y.mnRelocQuery,
                                      x.mnRelocWords, y.mnRelocWords, x.mRelocScore, y.mRelocScore, x.mnPlaceRecognitionQuery, y.mnPlaceRecognitionQuery,
                                      x.mnPlaceRecognitionWords, y.mnPlaceRecognitionWords, x.mPlaceRecognitionScore, y.mPlaceRecognitionScore);
        }
    }
}
static std::vector<long> Idx(World& w, const std::vector<KeyFrame*>& v) { std::vector<long> o; for (KeyFrame* k : v) o.push_back(k - w.kf.data()); return o; }
static void SameList(World& a, const std::vector<KeyFrame*>& x, World& b, const std::vector<KeyFrame*>& y, const char* what, int step) {
    if (Idx(a, x) != Idx(b, y) && g_fail++ < 10) printf("CANDIDATES %s step %d: %zu vs %zu\n", what, step, x.size(), y.size());
}

// One KeyFrameDatabase used by three threads at once, as Tracking (relocalisation), LoopClosing (loop / merge candidates) and LocalMapping (add, erase)
// use the reference's.  The writer's key frames hold only words of a reserved range that no query holds, so no candidate list can depend on how the
// threads interleave; the relocalisation thread alone touches the mnReloc* fields and the loop thread alone the mnPlaceRecognition* fields, so the
// restatement's answers are computed one call after the other, before the threads start.
static void ThreadedSection(const Voc& voc, int nwords, std::mt19937& g) {
    const int N = 300, kReserved = 64, kQueries = 20, kExtra = 24;
    const int world_words = nwords - kReserved;
    World A, B; std::mt19937 g2 = g; A.build(g, N, world_words); B.build(g2, N, world_words);
    KeyFrameDatabase db(voc); RestatedDB ref(nwords);
    for (int i = 0; i < N; i++) { db.add(&A.kf[i]); ref.add(&B.kf[i]); }
    std::vector<KeyFrame> extra(kExtra);
    std::uniform_real_distribution<double> u(0.05, 1.0);
    for (int i = 0; i < kExtra; i++) {
        extra[i].mnId = 9000 + i; extra[i].map = &A.maps[0];
        for (int j = 0; j < 30; j++) extra[i].mBowVec[(unsigned)(world_words + g() % kReserved)] = u(g);
        for (auto& kv : extra[i].mBowVec) if ((int)kv.first < world_words) { printf("THREADS a writer word is not in the reserved range\n"); g_fail++; }
    }
    struct Q { int src, map; };
    std::vector<Q> rq(kQueries), nq(kQueries);
    for (int s = 0; s < kQueries; s++) { rq[s] = {(int)(g() % N), s % 2}; nq[s] = {(int)(g() % N), 3}; }
    rq[5] = rq[4];                                                      // (ids below repeat too: 1 + s / 2)
    for (auto& k : A.kf) for (auto& kv : k.mBowVec) if ((int)kv.first >= world_words) { printf("THREADS a query word is in the writer's range\n"); g_fail++; return; }
    // the restatement, serially
    std::vector<std::vector<long> > er(kQueries), el(kQueries), em(kQueries), gr(kQueries), gl(kQueries), gm(kQueries);
    for (int s = 0; s < kQueries; s++) { Frame F; F.mnId = 1 + s / 2; F.mBowVec = B.kf[rq[s].src].mBowVec; er[s] = Idx(B, ref.Reloc(&F, &B.maps[rq[s].map])); }
    for (int s = 0; s < kQueries; s++) { std::vector<KeyFrame*> l, m; ref.NBest(&B.kf[nq[s].src], l, m, nq[s].map); el[s] = Idx(B, l); em[s] = Idx(B, m); }
    std::atomic<int> waiting(0), threw(0);
    auto barrier = [&] { waiting++; while (waiting.load() < 3) std::this_thread::yield(); };
    std::thread t_reloc([&] {
        barrier();
        try { for (int s = 0; s < kQueries; s++) { Frame F; F.mnId = 1 + s / 2; F.mBowVec = A.kf[rq[s].src].mBowVec; gr[s] = Idx(A, db.DetectRelocalizationCandidates(&F, &A.maps[rq[s].map])); } }
        catch (const std::exception& e) { printf("THREADS reloc: %s\n", e.what()); threw++; }
    });
    std::thread t_loop([&] {
        barrier();
        try { for (int s = 0; s < kQueries; s++) { std::vector<KeyFrame*> l, m; db.DetectNBestCandidates(&A.kf[nq[s].src], l, m, nq[s].map); gl[s] = Idx(A, l); gm[s] = Idx(A, m); } }
        catch (const std::exception& e) { printf("THREADS nbest: %s\n", e.what()); threw++; }
    });
    int writes = 0;
    std::thread t_write([&] {
        barrier();
        try {
            for (int round = 0; round < 3; round++) {
                for (int i = 0; i < kExtra; i++) { db.add(&extra[i]); writes++; if (i >= 4) { db.erase(&extra[i - 4]); writes++; } }
                for (int i = kExtra - 4; i < kExtra; i++) { db.erase(&extra[i]); writes++; }
            }
        } catch (const std::exception& e) { printf("THREADS writer: %s\n", e.what()); threw++; }
    });
    t_reloc.join(); t_loop.join(); t_write.join();
    g_fail += threw.load();
    size_t lists = 0;
    for (int s = 0; s < kQueries; s++) {
        if (gr[s] != er[s] && g_fail++ < 10) printf("THREADS reloc query %d: %zu candidates, the restatement has %zu\n", s, gr[s].size(), er[s].size());
        if ((gl[s] != el[s] || gm[s] != em[s]) && g_fail++ < 10) printf("THREADS nbest query %d: %zu + %zu candidates, the restatement has %zu + %zu\n", s, gl[s].size(), gm[s].size(), el[s].size(), em[s].size());
        lists += !er[s].empty() + !el[s].empty();
    }
    Same(A, B, "threads", 0);
    if (lists < (size_t)kQueries) { printf("THREADS only %zu candidate lists are not empty\n", lists); g_fail++; }
    printf("threads: queries=%d writes=%d lists=%zu size=%d\n", 2 * kQueries, writes, lists, orbv_db_size(db.Handle()));
    if (orbv_db_size(db.Handle()) != N) { printf("THREADS the writer's key frames are not all gone\n"); g_fail++; }
}

#ifndef KFDB_FACADE_TEST_NO_MAIN       // (tests/cpp/kfdb_gates_test.cpp includes this file for the mock world and the restatement)
int main(int argc, char** argv) {
    if (argc < 3) return 2;
    g_ref = ref_voc_load_text(argv[1]);
    orbx_extractor* h = ORBmatcher::SharedHandle();
    Voc voc;
    if (orbv_load_text(h, argv[1], &voc.v) != ORBX_OK) { printf("vocabulary: %s\n", orbx_last_error()); return 1; }
    const int nwords = orbv_words(voc.v);
    std::mt19937 g((unsigned)atoi(argv[2]));
    if (argc >= 6 && std::string(argv[3]) == "bench") {      // the restatement's relocalisation query on one core, ms per query
        const int N = atoi(argv[4]), Q = atoi(argv[5]);
        World w; w.build(g, N, nwords, 600, 400);          // ~1 000 words per key frame, like tools/bench_kfdb.py's maps
        RestatedDB r(nwords); for (auto& k : w.kf) r.add(&k);
        std::vector<double> ms;
        for (int q = 0; q < Q; q++) {
            Frame F; F.mnId = 1 + q; F.mBowVec = w.kf[g() % N].mBowVec;
            auto t0 = std::chrono::steady_clock::now(); auto c = r.Reloc(&F, &w.maps[0]); auto t1 = std::chrono::steady_clock::now();
            ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); (void)c;
        }
        std::sort(ms.begin(), ms.end());
        printf("BENCH n=%d median_ms=%.4f\n", N, ms[ms.size() / 2]);
        return 0;
    }
    const int N = 300;
    World A, B; std::mt19937 g2 = g; A.build(g, N, nwords); B.build(g2, N, nwords);
    KeyFrameDatabase db(voc); RestatedDB ref(nwords);
    for (int i = 0; i < N; i++) { db.add(&A.kf[i]); ref.add(&B.kf[i]); }
    db.add(&A.kf[5]); ref.add(&B.kf[5]);                    // a duplicate add
    int step = 0;
    auto reloc = [&](long unsigned id, int src, int map) {
        Frame Fa, Fb; Fa.mnId = Fb.mnId = id; Fa.mBowVec = Fb.mBowVec = A.kf[src].mBowVec;
        auto x = db.DetectRelocalizationCandidates(&Fa, &A.maps[map]); auto y = ref.Reloc(&Fb, &B.maps[map]);
        SameList(A, x, B, y, "reloc", step); Same(A, B, "reloc", step); step++;
        return x.size();
    };
    auto nbest = [&](int q, int n) {
        std::vector<KeyFrame*> la, ma, lb, mb;
        db.DetectNBestCandidates(&A.kf[q], la, ma, n); ref.NBest(&B.kf[q], lb, mb, n);
        SameList(A, la, B, lb, "nbest loop", step); SameList(A, ma, B, mb, "nbest merge", step); Same(A, B, "nbest", step); step++;
    };
    size_t nonempty = 0;
    for (int s = 0; s < 25; s++) nonempty += reloc(1 + s, (int)(g() % N), s % 2);
    reloc(7, 40, 0); reloc(7, 41, 0);                     // a repeat query id: counters grow on, stale scores
    reloc(8, 40, 0); reloc(9, 200, 0); reloc(8, 201, 0);
    for (int s = 0; s < 25; s++) nbest((int)(g() % N), 3);
    nbest(A.kf[30].mnId - 1000, 3); nbest(30, 3);         // the same key frame twice: same id
    for (int s = 0; s < 40; s++) { int e = (int)(g() % N); db.erase(&A.kf[e]); ref.erase(&B.kf[e]); }
    for (int s = 0; s < 10; s++) nonempty += reloc(100 + s, (int)(g() % N), 0);
    A.kf[10].map = &A.maps[1]; B.kf[10].map = &B.maps[1];  // moved to another map, then clearMap of that map
    db.clearMap(&A.maps[1]); ref.clearMap(&B.maps[1]);
    for (int s = 0; s < 10; s++) { nbest((int)(g() % N), 4); nonempty += reloc(200 + s, (int)(g() % N), 0); }
    for (int s = 0; s < N; s += 3) { A.kf[s].bad = B.kf[s].bad = true; }   // bad key frames in the candidate loop: no hang
    A.maps[2].bad = B.maps[2].bad = true;
    for (int s = 0; s < 10; s++) nbest((int)(g() % N), 3);
    bool threw = false;
    try { std::vector<KeyFrame*> l, m; db.DetectBestCandidates(&A.kf[0], l, m, 3); } catch (const std::runtime_error& e) { threw = std::string(e.what()).find("DetectBestCandidates") != std::string::npos; }
    if (!threw) { printf("DetectBestCandidates did not throw\n"); g_fail++; }
    db.clear(); ref = RestatedDB(nwords);
    reloc(999, 3, 0);
    ThreadedSection(voc, nwords, g);
    printf("steps=%d nonempty=%zu failures=%d\n", step, nonempty, g_fail);
    orbv_destroy(voc.v);
    return g_fail ? 1 : 0;
}
#endif
