// shared_objects_threads_test.cpp — one ORBVocabularyAmd (include/orb_slam3_amd/ORBVocabulary.h, on the emulator or the HIP library) shared by three
// std::threads, as Frame::ComputeBoW (Tracking) and KeyFrame::ComputeBoW (LocalMapping) share mpORBvocabulary: every thread calls
// transform(features, bow, fv, 4) on rows of its own, and every BowVector / FeatureVector must equal the one the reference's own DBoW2
// (oracle/_ref/libref_dbow2.so, ref_voc_transform) made of the same rows - computed serially, before the threads start.
// argv: vocabulary text file, calls per thread.  Last line: "calls=<n> failures=<n>".
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <thread>
#include <vector>
#include "ORBVocabulary.h"

extern "C" {
void* ref_voc_load_text(const char* path);
void ref_voc_transform(void* h, const void* desc, int n, int levelsup, void* bow_id, void* bow_val, int* n_bow, void* fv_node, void* fv_start, void* fv_feat, int* n_fv);
}

struct Rows {
    std::vector<cv::Mat> feats;
    DBoW2::BowVector bow; DBoW2::FeatureVector fv;       // the reference's
};

static const int kThreads = 3, kLevelsUp = 4;

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    void* ref = ref_voc_load_text(argv[1]);
    if (!ref) { printf("reference loadFromTextFile failed\n"); return 1; }
    const int calls = atoi(argv[2]);
    orbx_extractor* h = nullptr;
    if (orbx_create(&h, 500, 1.2f, 8, 20, 7, 0) != ORBX_OK) { printf("orbx_create: %s\n", orbx_last_error()); return 1; }
    ORB_SLAM3::ORBVocabularyAmd voc(h);
    if (!voc.loadFromTextFile(argv[1])) { printf("facade loadFromTextFile failed: %s\n", orbx_last_error()); return 1; }
    const int sizes[kThreads] = {700, 650, 500};
    Rows rows[kThreads];
    unsigned s = 2024;
    for (int t = 0; t < kThreads; t++) {
        const int n = sizes[t];
        std::vector<unsigned char> flat((size_t)n * 32);
        for (auto& b : flat) { s = s * 1664525u + 1013904223u; b = (unsigned char)(s >> 24); }
        rows[t].feats.resize(n);
        for (int i = 0; i < n; i++) { rows[t].feats[i].create(1, 32, CV_8U); memcpy(rows[t].feats[i].data, &flat[(size_t)i * 32], 32); }
        std::vector<unsigned> bi(n + 1), fn(n + 1), ff(n + 1); std::vector<double> bv(n + 1); std::vector<int> fs(n + 2);
        int nb = 0, nf = 0;
        ref_voc_transform(ref, flat.data(), n, kLevelsUp, bi.data(), bv.data(), &nb, fn.data(), fs.data(), ff.data(), &nf);
        for (int k = 0; k < nb; k++) rows[t].bow[bi[k]] = bv[k];
        for (int m = 0; m < nf; m++) rows[t].fv[fn[m]].assign(ff.begin() + fs[m], ff.begin() + fs[m + 1]);
        if (nb < 50 || nf < 2) { printf("thread %d: the reference's vectors are too small to tell anything (%d words, %d nodes)\n", t, nb, nf); return 1; }
    }
    {   // warm at the largest size
        DBoW2::BowVector b; DBoW2::FeatureVector f;
        voc.transform(rows[0].feats, b, f, kLevelsUp);
        if (!(static_cast<const std::map<DBoW2::WordId, DBoW2::WordValue>&>(b) == rows[0].bow)) { printf("the warming call differs from DBoW2\n"); return 1; }
    }
    std::atomic<int> waiting(0), failures(0), done(0);
    std::vector<std::thread> ths;
    for (int t = 0; t < kThreads; t++) {
        ths.emplace_back([&, t] {
            waiting++; while (waiting.load() < kThreads) std::this_thread::yield();        // the barrier
            for (int c = 0; c < calls; c++) {
                DBoW2::BowVector b; DBoW2::FeatureVector f;
                voc.transform(rows[t].feats, b, f, kLevelsUp);
                const bool same_b = static_cast<const std::map<DBoW2::WordId, DBoW2::WordValue>&>(b) == rows[t].bow;
                const bool same_f = static_cast<const std::map<DBoW2::NodeId, std::vector<unsigned int> >&>(f) == rows[t].fv;
                if (!same_b || !same_f) { if (failures++ < 10) printf("thread %d call %d: %s differs from DBoW2\n", t, c, same_b ? "FeatureVector" : "BowVector"); }
                done++;
            }
        });
    }
    for (auto& th : ths) th.join();
    printf("calls=%d failures=%d\n", done.load(), failures.load());
    return failures.load() ? 1 : 0;
}
