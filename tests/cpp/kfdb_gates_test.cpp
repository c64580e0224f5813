// kfdb_gates_test.cpp — include/orb_slam3_amd/KeyFrameDatabase.h on hand-built databases whose scores are CHOSEN, so that every comparison of the
// candidate selection stands at and beside equality.  Twin worlds (the mock world and RestatedDB of kfdb_facade_test.cpp): the facade answers on one, the
// restatement on the other, and both must give the candidate list WRITTEN with the scenario and equal query fields.
//
// How a score is chosen: the vocabulary scores L1 (DBoW2 ScoringObject.cpp, L1Scoring::score): -1/2 sum over the shared words of |q - d| - |q| - |d| =
// sum of min(q, d).  A query holds every one of its words at 8/64; a key frame that holds the shared words at a/64 <= 8/64 scores (sum of a) / 64 - a small
// dyadic number, exact in fp64 on the device and in the float the facade stores, and sums of a few of them are exact too: a score of 30/64 IS 0.75f * 40/64.
// argv: vocabulary text file (L1 scoring, >= 200 words) [, oracle/_ref/libkfdb_ref.so: the REFERENCE's own KeyFrameDatabase.cc over its own KeyFrame class
// (oracle/ref_kfdb_driver.cpp) as a third party - every operation is mirrored to it, and its candidate lists and query fields must be the written ones too]
#include <dlfcn.h>
#define KFDB_FACADE_TEST_NO_MAIN
#include "kfdb_facade_test.cpp"

namespace {

struct Spec {
    std::vector<int> vals;      // 64ths held at the query's words, from the first word on (0: the word is absent)
    std::vector<int> covis;     // indices of the best covisible key frames, best first
    int map;                    // 0: the query's map, 1: another map, 2: a bad map
};

const int kQueryBase = 20, kQueryWords = 10, kElsewhere = 100;

// the reference's database behind oracle/ref_kfdb_driver.cpp, when the driver was given the library
struct RefLib {
    void* (*create)(const char*, int) = nullptr;
    void (*sync)(void*, int, unsigned long, int, int, int, const unsigned*, const double*, int, const int*, const long*, const float*) = nullptr;
    void (*fields)(void*, int, long*, float*) = nullptr;
    void (*add)(void*, int) = nullptr; void (*erase)(void*, int) = nullptr; void (*clear_map)(void*, int) = nullptr;
    int (*reloc)(void*, unsigned long, int, const unsigned*, const double*, int, int*, int) = nullptr;
    void (*nbest)(void*, int, int, int*, int*, int*, int*, int) = nullptr;
    const char* vocabulary = nullptr;
    bool load(const char* path, const char* voc) {
        void* h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
        if (!h) { printf("dlopen: %s\n", dlerror()); return false; }
        vocabulary = voc;
        *(void**)&create = dlsym(h, "kr_create"); *(void**)&sync = dlsym(h, "kr_sync"); *(void**)&fields = dlsym(h, "kr_fields"); *(void**)&add = dlsym(h, "kr_add");
        *(void**)&erase = dlsym(h, "kr_erase"); *(void**)&clear_map = dlsym(h, "kr_clear_map"); *(void**)&reloc = dlsym(h, "kr_reloc"); *(void**)&nbest = dlsym(h, "kr_nbest");
        return create && sync && fields && add && erase && clear_map && reloc && nbest;
    }
} g_reference;
int g_reference_calls = 0;

struct Twin {
    World A, B;
    KeyFrameDatabase db; RestatedDB ref;
    void* third = nullptr;
    // the reference's key frames take what the restatement's twin holds now (equal to the facade's twin, or a failure has been printed)
    void sync() {
        if (!third) return;
        for (size_t i = 0; i < B.kf.size(); i++) {
            const KeyFrame& k = B.kf[i];
            std::vector<unsigned> ids; std::vector<double> vals; std::vector<int> covis;
            for (auto& kv : k.mBowVec) { ids.push_back(kv.first); vals.push_back(kv.second); }
            for (KeyFrame* c : k.covis) covis.push_back((int)(c - B.kf.data()));
            const long q[4] = {(long)k.mnRelocQuery, k.mnRelocWords, (long)k.mnPlaceRecognitionQuery, k.mnPlaceRecognitionWords}; const float s[2] = {k.mRelocScore, k.mPlaceRecognitionScore};
            g_reference.sync(third, (int)i, k.mnId, (int)(k.map - B.maps), k.map->bad, (int)ids.size(), ids.data(), vals.data(), (int)covis.size(), covis.data(), q, s);
        }
    }
    // ... and afterwards hold what the facade's twin holds
    void same_fields(const char* what) {
        if (!third) return;
        for (size_t i = 0; i < A.kf.size(); i++) {
            long q[4]; float s[2]; g_reference.fields(third, (int)i, q, s);
            const KeyFrame& k = A.kf[i];
            if (q[0] != (long)k.mnRelocQuery || q[1] != k.mnRelocWords || q[2] != (long)k.mnPlaceRecognitionQuery || q[3] != k.mnPlaceRecognitionWords || s[0] != k.mRelocScore || s[1] != k.mPlaceRecognitionScore) {
                printf("GATE %s: key frame %zu: the reference holds %ld %ld %ld %ld %a %a, the facade %lu %d %lu %d %a %a\n", what, i, q[0], q[1], q[2], q[3], s[0], s[1], k.mnRelocQuery, k.mnRelocWords,
                       k.mnPlaceRecognitionQuery, k.mnPlaceRecognitionWords, k.mRelocScore, k.mPlaceRecognitionScore);
                g_fail++;
            }
        }
    }
    Twin(const Voc& voc, int nwords, const std::vector<Spec>& specs) : db(voc), ref(nwords) {
        if (g_reference.create) { third = g_reference.create(g_reference.vocabulary, (int)specs.size()); if (!third) { printf("the reference's vocabulary did not load\n"); g_fail++; } }
        for (World* w : {&A, &B}) {
            w->kf.assign(specs.size(), KeyFrame());
            w->maps[2].bad = true;
            for (size_t i = 0; i < specs.size(); i++) {
                KeyFrame& k = w->kf[i];
                k.mnId = 1000 + i; k.map = &w->maps[specs[i].map];
                for (size_t j = 0; j < specs[i].vals.size(); j++) if (specs[i].vals[j]) k.mBowVec[kQueryBase + (unsigned)j] = specs[i].vals[j] / 64.0;
                if (k.mBowVec.empty()) k.mBowVec[kElsewhere + (unsigned)i] = 0.5;       // a key frame that shares nothing with the query
                for (int c : specs[i].covis) k.covis.push_back(&w->kf[c]);
            }
        }
    }
    void add(int i) { db.add(&A.kf[i]); ref.add(&B.kf[i]); if (third) { sync(); g_reference.add(third, i); } }
    void addAll() { for (size_t i = 0; i < A.kf.size(); i++) add((int)i); }
    void erase(int i) { db.erase(&A.kf[i]); ref.erase(&B.kf[i]); if (third) { sync(); g_reference.erase(third, i); } }
    void clearMap(int m) { db.clearMap(&A.maps[m]); ref.clearMap(&B.maps[m]); if (third) { sync(); g_reference.clear_map(third, m); } }
    template <class F> void both(F f) { f(A); f(B); }
};

Bow QueryBow(int words = kQueryWords, int first = 0) { Bow b; for (int j = first; j < first + words; j++) b[kQueryBase + (unsigned)j] = 8 / 64.0; return b; }

std::string Str(const std::vector<long>& v) { std::string s = "["; for (long x : v) s += (s.size() > 1 ? " " : "") + std::to_string(x); return s + "]"; }

void Expect(const char* what, const std::vector<long>& facade, const std::vector<long>& restated, const std::vector<long>& written) {
    if (facade != written || restated != written) { printf("GATE %s: facade %s, restatement %s, written %s\n", what, Str(facade).c_str(), Str(restated).c_str(), Str(written).c_str()); g_fail++; }
}
void ExpectInt(const char* what, long facade, long restated, long written) {
    if (facade != written || restated != written) { printf("GATE %s: facade %ld, restatement %ld, written %ld\n", what, facade, restated, written); g_fail++; }
}

const std::vector<long> kAgree = {-999};
std::vector<long> Reloc(Twin& t, const char* what, long unsigned id, const Bow& bow, int map, const std::vector<long>& written_) {
    Frame Fa, Fb; Fa.mnId = Fb.mnId = id; Fa.mBowVec = Fb.mBowVec = bow;
    t.sync();
    const std::vector<long> x = Idx(t.A, t.db.DetectRelocalizationCandidates(&Fa, &t.A.maps[map])), y = Idx(t.B, t.ref.Reloc(&Fb, &t.B.maps[map]));
    const std::vector<long> written = written_ == kAgree ? x : written_;          // (the random worlds: no table, the three must agree)
    Expect(what, x, y, written); Same(t.A, t.B, what, 0);
    if (t.third) {
        std::vector<unsigned> ids; std::vector<double> vals; for (auto& kv : bow) { ids.push_back(kv.first); vals.push_back(kv.second); }
        int out[32]; const int n = g_reference.reloc(t.third, id, (int)ids.size(), ids.data(), vals.data(), map, out, 32);
        const std::vector<long> z(out, out + (n < 32 ? n : 32));
        Expect((std::string(what) + ", the reference's KeyFrameDatabase.cc").c_str(), z, z, written); t.same_fields(what); g_reference_calls++;
    }
    return x;
}
void NBest(Twin& t, const char* what, int q, int n, const std::vector<long>& loop_, const std::vector<long>& merge_) {
    std::vector<KeyFrame*> la, ma, lb, mb;
    t.sync();
    t.db.DetectNBestCandidates(&t.A.kf[q], la, ma, n); t.ref.NBest(&t.B.kf[q], lb, mb, n);
    const std::vector<long> loop = loop_ == kAgree ? Idx(t.A, la) : loop_, merge = merge_ == kAgree ? Idx(t.A, ma) : merge_;
    Expect((std::string(what) + ", loop").c_str(), Idx(t.A, la), Idx(t.B, lb), loop);
    Expect((std::string(what) + ", merge").c_str(), Idx(t.A, ma), Idx(t.B, mb), merge);
    Same(t.A, t.B, what, 0);
    if (t.third) {
        int l[32], m[32], nl = 0, nm = 0; g_reference.nbest(t.third, q, n, l, &nl, m, &nm, 32);
        const std::vector<long> zl(l, l + (nl < 32 ? nl : 32)), zm(m, m + (nm < 32 ? nm : 32));
        Expect((std::string(what) + ", loop, the reference's KeyFrameDatabase.cc").c_str(), zl, zl, loop);
        Expect((std::string(what) + ", merge, the reference's KeyFrameDatabase.cc").c_str(), zm, zm, merge); t.same_fields(what); g_reference_calls++;
    }
}

std::vector<int> V(int a, int n) { return std::vector<int>(n, a); }
std::vector<int> V(int a, int n, int b, int m, int c = 0, int l = 0) { std::vector<int> v(n, a); v.insert(v.end(), m, b); v.insert(v.end(), l, c); return v; }

// The lines of the group selection.  minCommonWords = (int)(10 * 0.8f) = 8.  In 64ths:
//   k0 20, neighbour k1 (12): 32, leads itself          k1 12, neighbour k4 - not stamped by this query, its stale score 64/64 must not be added: 12
//   k2 30 with 9 words: 30 == 0.75f * 40 exactly: out   k3 31 with 9 words: in
//   k5 20, neighbour k0 with the SAME score 20: 40, the best; k5 leads its group (the neighbour's score is not larger)
//   k6 64 with 8 words == minCommonWords: never scored  k7 shares 5 words: stamped and counted, never scored, no group
const std::vector<Spec> kLines = {
    {V(2, 10), {1}, 0}, {V(1, 8, 2, 2), {4}, 0}, {V(3, 6, 4, 3), {}, 0}, {V(3, 6, 4, 2, 5, 1), {}, 0}, {{}, {}, 0}, {V(2, 10), {0}, 0}, {V(8, 8), {}, 0}, {V(1, 5, 0, 5), {5}, 0}};

void RelocLines(const Voc& voc, int nwords) {
    Twin t(voc, nwords, kLines);
    t.both([](World& w) { w.kf[4].mRelocScore = 1.0f; w.kf[4].mnRelocQuery = 77; w.kf[1].mnRelocWords = 3; w.kf[1].mnRelocQuery = 77; });
    t.addAll();
    // accumulated: k0 32, k1 12, k2 30, k3 31, k5 40; kept above 0.75f * 40 = 30, in the order of the walk
    Reloc(t, "reloc, the lines", 1, QueryBow(), 0, {0, 3, 5});
    const int words[8] = {10, 10, 9, 9, 0, 10, 8, 5};
    const float score[8] = {20 / 64.f, 12 / 64.f, 30 / 64.f, 31 / 64.f, 1.0f, 20 / 64.f, 0.f, 0.f};
    for (int i = 0; i < 8; i++) {
        ExpectInt("reloc, the lines: mnRelocWords", t.A.kf[i].mnRelocWords, t.B.kf[i].mnRelocWords, words[i]);
        if (t.A.kf[i].mRelocScore != score[i]) { printf("GATE reloc, the lines: mRelocScore of %d is %a, written %a\n", i, t.A.kf[i].mRelocScore, score[i]); g_fail++; }
    }
}

// k0 10 with the neighbours k1 (30) and k2 (20): the first raises the group's best score to 30, so the second does not take the lead.  60 / 30 / 20: only the first group is above 45
void RelocBestScoreIsRaised(const Voc& voc, int nwords) {
    Twin t(voc, nwords, {{V(1, 10), {1, 2}, 0}, {V(3, 10), {}, 0}, {V(2, 10), {}, 0}});
    t.addAll();
    Reloc(t, "reloc, the best score is raised", 2, QueryBow(), 0, {1});
}

// k0 20 + k1 30 = 50 led by k1, which lies in another map: dropped.  k2 25 + k3 40 = 65 led by k3.  k3 alone 40: below 0.75f * 65.  k4 10 + k3 40 = 50 led by k3 again: listed once
void RelocMapAndDuplicates(const Voc& voc, int nwords) {
    Twin t(voc, nwords, {{V(2, 10), {1}, 0}, {V(3, 10), {}, 1}, {V(2, 5, 3, 5), {3}, 0}, {V(4, 10), {}, 0}, {V(1, 10), {3}, 0}});
    t.addAll();
    Reloc(t, "reloc, map and duplicates", 3, QueryBow(), 0, {3});
}

// A repeat query id.  The first query (ten words) stamps k0 alone.  The second, under the same id, holds those ten words and seven more: k0 is stamped already - not
// listed, its counter grows to 20 - and k1 shares the seven.  The device sees 10 and 7 shared words and scores above (int)(10 * 0.8f) = 8: not k1.  The host's list
// holds k1 alone, minCommonWords = (int)(7 * 0.8f) = 5, and k1 is a candidate: its score has to be asked for again
void RelocRepeatId(const Voc& voc, int nwords) {
    Twin t(voc, nwords, {{V(2, 10), {}, 0}, {V(0, 10, 2, 7), {}, 0}});
    t.addAll();
    Reloc(t, "reloc, first query of the id", 9, QueryBow(), 0, {0});
    Reloc(t, "reloc, the id again", 9, QueryBow(17), 0, {1});
    ExpectInt("reloc, the id again: k0's counter grows on", t.A.kf[0].mnRelocWords, t.B.kf[0].mnRelocWords, 20);
    ExpectInt("reloc, the id again: k1's counter", t.A.kf[1].mnRelocWords, t.B.kf[1].mnRelocWords, 7);
}

// the query key frame is the last of the world; it is not in the database
std::vector<Spec> WithQuery(std::vector<Spec> s, const std::vector<int>& connected = {}) { s.push_back({V(8, 10), connected, 0}); return s; }

// the repeat id of DetectNBestCandidates: the same key frame asks twice, and its BoW vector has grown by seven words in between (KeyFrame::ComputeBoW ran again).
// As in RelocRepeatId: k0 is stamped, its counter grows to 20; k1 shares the seven new words and is the one candidate, scored by the second question
void NBestRepeatId(const Voc& voc, int nwords) {
    Twin t(voc, nwords, WithQuery({{V(2, 10), {}, 0}, {V(0, 10, 2, 7), {}, 0}}));
    t.add(0); t.add(1);
    NBest(t, "nbest, first query of the id", 2, 3, {0}, {});
    t.both([](World& w) { w.kf[2].mBowVec = QueryBow(17); });
    NBest(t, "nbest, the id again", 2, 3, {1}, {});
    ExpectInt("nbest, the id again: k0's counter grows on", t.A.kf[0].mnPlaceRecognitionWords, t.B.kf[0].mnPlaceRecognitionWords, 20);
}

// the same groups through DetectNBestCandidates: no 0.75 filter, a sort instead.  40 (k5), 32 (k0), 31 (k3), 30 (k2), 25 (k7's group, led by k5: a duplicate), 12 (k1)
void NBestLines(const Voc& voc, int nwords) {
    std::vector<Spec> s = kLines;
    s[7] = {V(1, 5, 0, 5), {5}, 0};
    Twin t(voc, nwords, WithQuery(s));
    t.both([](World& w) { w.kf[4].mPlaceRecognitionScore = 1.0f; w.kf[4].mnPlaceRecognitionQuery = 77; w.kf[1].mnPlaceRecognitionWords = 3; w.kf[1].mnPlaceRecognitionQuery = 77; });
    for (int i = 0; i < 8; i++) t.add(i);
    // k7 shares five words: below minCommonWords, not scored - its group does not exist, and k5 is listed once anyway
    NBest(t, "nbest, the lines", 8, 10, {5, 0, 3, 2, 1}, {});
    ExpectInt("nbest, the lines: k1's counter was reset", t.A.kf[1].mnPlaceRecognitionWords, t.B.kf[1].mnPlaceRecognitionWords, 10);
    ExpectInt("nbest, the lines: k6 holds exactly minCommonWords", t.A.kf[6].mnPlaceRecognitionWords, t.B.kf[6].mnPlaceRecognitionWords, 8);
    if (t.A.kf[6].mPlaceRecognitionScore != 0.f) { printf("GATE nbest, the lines: k6 was scored\n"); g_fail++; }
}

// two groups with one leader, both scored: k0 10 + k1 30 = 40 led by k1; k1 alone 30; k2 9 + k1 30 = 39 led by k1.  Sorted 40, 39, 30: k1 once
void NBestDuplicates(const Voc& voc, int nwords) {
    Twin t(voc, nwords, WithQuery({{V(1, 10), {1}, 0}, {V(3, 10), {}, 0}, {V(1, 9, 0, 1), {1}, 0}}));
    for (int i = 0; i < 3; i++) t.add(i);
    NBest(t, "nbest, duplicates", 3, 10, {1}, {});
}

// equal accumulated scores keep the order of the walk (std::list::sort is stable): 30 k1 (other map), 30 k4, 20 k0, 20 k2, 20 k3 (other map), 20 k5 (bad map).
// two of each: k1 merge, k4 loop, k0 loop, k2 - the loop list is full, and a key frame of the query's map is no merge candidate -, k3 merge: both full
void NBestStableSort(const Voc& voc, int nwords) {
    Twin t(voc, nwords, WithQuery({{V(2, 10), {}, 0}, {V(3, 10), {}, 1}, {V(2, 10), {}, 0}, {V(2, 10), {}, 1}, {V(3, 10), {}, 0}, {V(2, 10), {}, 2}}));
    for (int i = 0; i < 6; i++) t.add(i);
    NBest(t, "nbest, equal scores", 6, 2, {4, 0}, {1, 3});
}

// nNumCandidates reached on the merge side only, and a bad map on the merge side: 20 k0 (bad map: no candidate, though the merge list is empty), 19 k1, 18 k2: the merge
// list is full; 17 k3 (other map: one too many); 16 k4, 15 k5: the walk goes on until the loop list is full too
void NBestOneSideFull(const Voc& voc, int nwords) {
    Twin t(voc, nwords, WithQuery({{V(2, 10), {}, 2}, {V(2, 9, 1, 1), {}, 1}, {V(2, 8, 1, 2), {}, 1}, {V(2, 7, 1, 3), {}, 1}, {V(2, 6, 1, 4), {}, 0}, {V(2, 5, 1, 5), {}, 0}}));
    for (int i = 0; i < 6; i++) t.add(i);
    NBest(t, "nbest, one side full", 6, 2, {4, 5}, {1, 2});
}

// The connected key frames' counter.  They are excluded from the query and never stamped; the reference's walk resets their counter at every list entry and counts one:
//   k1 connected, added TWICE, shares 4 words: ends at 1        k2 connected, in the database, shares nothing: untouched (7 from an earlier query)
//   k3 connected, not in the database, shares 10 words: untouched (7)
//   k4 connected, added twice, shares 3 words, and stamped with this id by an earlier query (counter 5): every list entry counts, 5 + 2 * 3 = 11
// k0 is the one candidate
void NBestConnected(const Voc& voc, int nwords) {
    Twin t(voc, nwords, WithQuery({{V(2, 10), {}, 0}, {V(2, 4, 0, 6), {}, 0}, {{}, {}, 0}, {V(2, 10), {}, 0}, {V(2, 3, 0, 7), {}, 0}}, {1, 2, 3, 4}));
    const long unsigned id = t.A.kf[5].mnId;
    t.both([&](World& w) { w.kf[2].mnPlaceRecognitionWords = 7; w.kf[3].mnPlaceRecognitionWords = 7; w.kf[4].mnPlaceRecognitionWords = 5; w.kf[4].mnPlaceRecognitionQuery = id; });
    t.add(0); t.add(1); t.add(1); t.add(2); t.add(4); t.add(4);
    NBest(t, "nbest, connected key frames", 5, 3, {0}, {});
    const int words[5] = {10, 1, 7, 7, 11};
    for (int i = 0; i < 5; i++) ExpectInt("nbest, connected key frames: mnPlaceRecognitionWords", t.A.kf[i].mnPlaceRecognitionWords, t.B.kf[i].mnPlaceRecognitionWords, words[i]);
    for (int i = 1; i < 4; i++) ExpectInt("nbest, connected key frames: never stamped", (long)t.A.kf[i].mnPlaceRecognitionQuery, (long)t.B.kf[i].mnPlaceRecognitionQuery, 0);
}

// A key frame added twice and erased once is still in the database, once: a query counts its words once, clearMap of its map takes it out, and as a connected key
// frame it still gets the 1.  Then a key frame whose GetMap() changed after add: clearMap asks at the moment of the call
void AddEraseClearMap(const Voc& voc, int nwords) {
    Twin t(voc, nwords, WithQuery({{V(2, 10), {}, 0}, {V(2, 10), {}, 0}, {V(2, 10), {}, 1}}, {0}));      // 20 each: all above 0.75f * 20
    t.add(0); t.add(0); t.add(1); t.add(2);
    t.erase(0);
    Reloc(t, "added twice, erased once", 1, QueryBow(), 0, {0, 1});
    ExpectInt("added twice, erased once: counted once", t.A.kf[0].mnRelocWords, t.B.kf[0].mnRelocWords, 10);
    if (orbv_db_size(t.db.Handle()) != 3) { printf("GATE added twice, erased once: the database holds %d key frames\n", orbv_db_size(t.db.Handle())); g_fail++; }
    NBest(t, "added twice, erased once, connected", 3, 3, {1}, {2});
    ExpectInt("added twice, erased once, connected: the counter", t.A.kf[0].mnPlaceRecognitionWords, t.B.kf[0].mnPlaceRecognitionWords, 1);
    t.both([](World& w) { w.kf[1].map = &w.maps[1]; });            // k1 moves to the other map after its add
    t.clearMap(1);                                                  // k1 and k2 go, k0 stays
    if (orbv_db_size(t.db.Handle()) != 1) { printf("GATE clearMap after GetMap() changed: the database holds %d key frames\n", orbv_db_size(t.db.Handle())); g_fail++; }
    Reloc(t, "clearMap after GetMap() changed", 2, QueryBow(), 0, {0});
    t.clearMap(0);
    if (orbv_db_size(t.db.Handle()) != 0) { printf("GATE clearMap of the last map: the database holds %d key frames\n", orbv_db_size(t.db.Handle())); g_fail++; }
    Reloc(t, "an empty database", 3, QueryBow(), 0, {});
}

// the random twin worlds of kfdb_facade_test.cpp, 60 key frames, through all three: relocalisation and loop / merge queries with repeat ids, erasures, a key frame
// that changes maps and clearMap.  No bad key frame: the reference does not advance past one in the candidate loop of DetectNBestCandidates and spins
void RandomWorlds(const Voc& voc, int nwords, unsigned seed) {
    const int N = 60;
    Twin t(voc, nwords, std::vector<Spec>(N, Spec{{}, {}, 0}));
    std::mt19937 g(seed), g2 = g;
    t.A.build(g, N, nwords, 24, 6); t.B.build(g2, N, nwords, 24, 6);
    t.addAll(); t.add(5);
    size_t nonempty = 0;
    for (int s = 0; s < 12; s++) nonempty += Reloc(t, "random reloc", 1 + s / 2, t.A.kf[g() % N].mBowVec, s % 2, kAgree).size();
    for (int s = 0; s < 12; s++) NBest(t, "random nbest", (int)(g() % N), 3, kAgree, kAgree);
    NBest(t, "random nbest", 30, 3, kAgree, kAgree); NBest(t, "random nbest, the id again", 30, 3, kAgree, kAgree);
    for (int s = 0; s < 10; s++) t.erase((int)(g() % N));
    t.both([](World& w) { w.kf[10].map = &w.maps[1]; });
    t.clearMap(1);
    for (int s = 0; s < 8; s++) { NBest(t, "random nbest after clearMap", (int)(g() % N), 4, kAgree, kAgree); nonempty += Reloc(t, "random reloc after clearMap", 100 + s, t.A.kf[g() % N].mBowVec, 0, kAgree).size(); }
    if (nonempty < 5) { printf("GATE random worlds: %zu candidates in all\n", nonempty); g_fail++; }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    g_ref = ref_voc_load_text(argv[1]);
    Voc voc;
    if (orbv_load_text(ORBmatcher::SharedHandle(), argv[1], &voc.v) != ORBX_OK) { printf("vocabulary: %s\n", orbx_last_error()); return 1; }
    const int nwords = orbv_words(voc.v);
    if (argc > 2 && !g_reference.load(argv[2], argv[1])) { printf("the reference library did not load\n"); return 1; }
    if (nwords < 200) { printf("the vocabulary holds %d words\n", nwords); return 1; }
    RelocLines(voc, nwords);
    RelocBestScoreIsRaised(voc, nwords);
    RelocMapAndDuplicates(voc, nwords);
    RelocRepeatId(voc, nwords);
    NBestRepeatId(voc, nwords);
    NBestLines(voc, nwords);
    NBestDuplicates(voc, nwords);
    NBestStableSort(voc, nwords);
    NBestOneSideFull(voc, nwords);
    NBestConnected(voc, nwords);
    AddEraseClearMap(voc, nwords);
    for (int a = 3; a < argc; a++) RandomWorlds(voc, nwords, (unsigned)atoi(argv[a]));          // [seeds of random twin worlds]
    printf("scenarios=11 reference_calls=%d failures=%d\n", g_reference_calls, g_fail);
    orbv_destroy(voc.v);
    return g_fail ? 1 : 0;
}
