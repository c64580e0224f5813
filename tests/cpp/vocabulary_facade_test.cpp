// tests/cpp/vocabulary_facade_test.cpp — TEST ONLY.  One binary holds the reference's own DBoW2 (compiled from /root/reference) and the
// facade include/orb_slam3_amd/ORBVocabulary.h on top of the product C ABI; both load the same vocabulary text file and transform the
// same descriptors; the resulting DBoW2::BowVector / FeatureVector objects must be equal (operator== of std::map: ids, doubles, order).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "DBoW2/FORB.h"
#include "DBoW2/TemplatedVocabulary.h"
#include "ORBVocabulary.h"

typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> RefVocabulary;

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s voc.txt n_features\n", argv[0]); return 2; }
    const int n = atoi(argv[2]);
    RefVocabulary ref;
    if (!ref.loadFromTextFile(argv[1])) { fprintf(stderr, "reference loadFromTextFile failed\n"); return 1; }
    orbx_extractor* h = nullptr;
    if (orbx_create(&h, 500, 1.2f, 8, 20, 7, 0) != ORBX_OK) { fprintf(stderr, "orbx_create: %s\n", orbx_last_error()); return 1; }
    ORB_SLAM3::ORBVocabularyAmd voc(h);
    if (!voc.loadFromTextFile(argv[1])) { fprintf(stderr, "facade loadFromTextFile failed: %s\n", orbx_last_error()); return 1; }
    if (voc.size() != ref.size()) { fprintf(stderr, "size %u vs %u\n", voc.size(), ref.size()); return 1; }
    unsigned s = 12345;
    for (int round = 0; round < 4; round++) {
        const int m = round == 3 ? 0 : n - 7 * round;
        std::vector<cv::Mat> feats(m);
        for (int i = 0; i < m; i++) {
            feats[i].create(1, 32, CV_8U);
            for (int b = 0; b < 32; b++) { s = s * 1664525u + 1013904223u; feats[i].data[b] = (unsigned char)(s >> 24); }
        }
        for (int levelsup = 0; levelsup <= 4; levelsup += 2) {
            DBoW2::BowVector bv1, bv2; DBoW2::FeatureVector fv1, fv2;
            bv1[0xFFFFF0u] = 1.0; bv2[0xFFFFF0u] = 1.0; fv1[0xFFFFF0u].push_back(1); fv2[0xFFFFF0u].push_back(1);      // transform clears what the vectors held (TemplatedVocabulary.h:1132-1133)
            ref.transform(feats, bv1, fv1, levelsup);
            voc.transform(feats, bv2, fv2, levelsup);
            if (!(static_cast<const std::map<DBoW2::WordId, DBoW2::WordValue>&>(bv1) == bv2)) { fprintf(stderr, "BowVector differs (round %d, levelsup %d)\n", round, levelsup); return 1; }
            if (!(static_cast<const std::map<DBoW2::NodeId, std::vector<unsigned int> >&>(fv1) == fv2)) { fprintf(stderr, "FeatureVector differs (round %d, levelsup %d)\n", round, levelsup); return 1; }
            if (m > 50 && bv1.size() < 10) { fprintf(stderr, "suspiciously small BowVector\n"); return 1; }
        }
    }
    // a second load replaces the device vocabulary: after the same transform as before it, nothing more is allocated than there was
    {
        std::vector<cv::Mat> feats(n);
        for (int i = 0; i < n; i++) { feats[i].create(1, 32, CV_8U); for (int b = 0; b < 32; b++) { s = s * 1664525u + 1013904223u; feats[i].data[b] = (unsigned char)(s >> 24); } }
        DBoW2::BowVector bv1, bv2; DBoW2::FeatureVector fv1, fv2;
        long long before[4], after[4];
        voc.transform(feats, bv1, fv1, 4);
        orbx_debug_live_resources(before);
        if (!voc.loadFromTextFile(argv[1]) || voc.size() != ref.size()) { fprintf(stderr, "the second loadFromTextFile failed\n"); return 1; }
        voc.transform(feats, bv2, fv2, 4);
        orbx_debug_live_resources(after);
        if (!(static_cast<const std::map<DBoW2::WordId, DBoW2::WordValue>&>(bv1) == bv2) || bv1.empty()) { fprintf(stderr, "BowVector differs after the second load\n"); return 1; }
        if (after[0] != before[0]) { fprintf(stderr, "a second load left %lld device allocations behind\n", after[0] - before[0]); return 1; }
    }
    orbx_destroy(h);
    printf("ok\n");
    return 0;
}
