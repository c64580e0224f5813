// ORBmatcher::ResidentKeyFrames::Adopt / ORBmatcher::AdoptImplicit (include/orb_slam3_amd/ORBmatcher.h): a key frame made on the device
// (orbm_keyframe_create_extracted) enters the cache of resident key frames under the tag Get computes, so that a search naming the host object uploads
// nothing.  A mock key frame carries the members the facade reads, under the reference's names, filled from orbm_keyframe_fetch of the device-made
// key frame.  Checked: Get returns the adopted object and neither the cache nor the library's count of device allocations changes; Adopt over an entry
// destroys the old object; Erase frees; a host object whose mFeatVec has changed since (ComputeBoW ran) makes Get rebuild.  Prints "ADOPT OK".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>
#include "orb_slam3_amd/ORBmatcher.h"

namespace {

struct MockKeyFrame {
    long unsigned int mnId = 7;
    int N = 0, NLeft = -1;
    void* mpCamera2 = nullptr;
    std::vector<cv::KeyPoint> mvKeysUn, mvKeys, mvKeysRight;
    cv::Mat mDescriptors;
    std::vector<float> mvuRight, mvScaleFactors, mvLevelSigma2;
    std::map<unsigned, std::vector<unsigned> > mFeatVec;
};
typedef ORB_SLAM3::ORBmatcher::ResidentKeyFrames<MockKeyFrame> Cache;

int failures = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)
#define OK(call) do { const int rc_ = (call); if (rc_ != ORBX_OK) { printf("line %d: %s -> %d (%s)\n", __LINE__, #call, rc_, orbx_last_error()); exit(2); } } while (0)

long long device_allocations() { long long l[4]; OK(orbx_debug_live_resources(l)); return l[0]; }

}  // namespace

int main() {
    const int W = 376, H = 240;
    std::mt19937 rng(5);
    std::vector<uint8_t> img((size_t)W * H, 90);
    for (int r = 0; r < 700; r++) {                                // rectangles of random grey: corners everywhere
        const int x0 = (int)(rng() % (W - 8)), y0 = (int)(rng() % (H - 8)), w = 6 + (int)(rng() % 40), h = 6 + (int)(rng() % 40);
        const uint8_t g = (uint8_t)(rng() % 256);
        for (int y = y0; y < y0 + h && y < H; y++) for (int x = x0; x < x0 + w && x < W; x++) img[(size_t)y * W + x] = g;
    }
    orbx_extractor* ex = nullptr;
    OK(orbx_create(&ex, 500, 1.2f, 8, 20, 7, 0));
    OK(orbx_extract_batch(ex, 1, img.data(), W, H, W, (size_t)W * H, 0, 0, 0));
    // a vocabulary of two levels, three children per node
    const int k = 3, L = 2, n_nodes = k + k * k;
    std::vector<int> parent; std::vector<uint8_t> leaf, desc((size_t)n_nodes * 32); std::vector<double> weight;
    for (int a = 0; a < k; a++) { parent.push_back(0); leaf.push_back(0); weight.push_back(0.0); }
    for (int a = 0; a < k; a++) for (int c = 0; c < k; c++) { parent.push_back(a + 1); leaf.push_back(1); weight.push_back(c == 2 && a == 1 ? 0.0 : 1.0 + c); }
    for (size_t i = 0; i < desc.size(); i++) desc[i] = (uint8_t)(rng() % 256);
    orbv_vocabulary* voc = nullptr;
    OK(orbv_create(ex, k, L, 0, 0, n_nodes, parent.data(), leaf.data(), desc.data(), weight.data(), &voc));
    OK(orbv_transform_extracted(voc, ex, 0, 1, 1));
    const int frame0 = 0;
    orbm_keyframe *dev = nullptr, *dev2 = nullptr, *dev3 = nullptr, *dev4 = nullptr;
    OK(orbm_keyframe_create_extracted(ex, voc, 1, &frame0, 0, &dev));
    OK(orbm_keyframe_create_extracted(ex, voc, 1, &frame0, 0, &dev2));
    OK(orbm_keyframe_create_extracted(ex, voc, 1, &frame0, 0, &dev3));
    OK(orbm_keyframe_create_extracted(ex, voc, 1, &frame0, 0, &dev4));
    // the host object, as Tracking::CreateNewKeyFrame would hold it had the frame come down: from the key frame's own arrays
    MockKeyFrame kf;
    int N = 0, nodes = 0;
    OK(orbm_keyframe_fetch(ex, dev, &N, &nodes, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    EXPECT(N > 100 && nodes >= 2);
    std::vector<OrbxKeyPoint> keys(N); std::vector<uint32_t> fnode(nodes), ffeat(N); std::vector<int> fstart(nodes + 1);
    kf.N = N; kf.mDescriptors.create(N, 32, CV_8UC1); kf.mvuRight.assign(N, -1.0f);
    OK(orbm_keyframe_fetch(ex, dev, nullptr, nullptr, keys.data(), kf.mDescriptors.ptr(0), nullptr, fnode.data(), fstart.data(), ffeat.data(), nullptr));
    for (int i = 0; i < N; i++) kf.mvKeysUn.push_back(cv::KeyPoint(keys[i].x, keys[i].y, keys[i].size, keys[i].angle, keys[i].response, keys[i].octave, keys[i].class_id));
    for (int a = 0; a < nodes; a++) kf.mFeatVec[fnode[a]] = std::vector<unsigned>(ffeat.begin() + fstart[a], ffeat.begin() + fstart[a + 1]);
    float s = 1.0f;
    for (int l = 0; l < 8; l++) { kf.mvScaleFactors.push_back(s); kf.mvLevelSigma2.push_back(s * s); s *= 1.2f; }

    {
        Cache cache;
        // Adopt, then Get: the adopted object, nothing uploaded, nothing allocated
        cache.Adopt(&kf, dev);
        EXPECT(cache.size() == 1);
        const long long live0 = device_allocations();
        EXPECT(cache.Get(&kf) == dev && cache.Get(&kf) == dev);
        EXPECT(cache.size() == 1 && device_allocations() == live0);
        // Adopt over an entry: the cache destroys the object it held
        cache.Adopt(&kf, dev2);
        EXPECT(cache.size() == 1 && device_allocations() == live0 - 1);
        EXPECT(cache.Get(&kf) == dev2);
        cache.Adopt(&kf, dev2);                                    // the same object again: kept
        EXPECT(cache.Get(&kf) == dev2 && device_allocations() == live0 - 1);
        // Erase frees it
        cache.Erase(&kf);
        EXPECT(cache.size() == 0 && device_allocations() == live0 - 2);
        // a tag that no longer fits: ComputeBoW ran on the host object after the adoption - Get rebuilds from the host arrays
        std::map<unsigned, std::vector<unsigned> > full = kf.mFeatVec;
        kf.mFeatVec.erase(kf.mFeatVec.begin());
        cache.Adopt(&kf, dev3);
        EXPECT(cache.Get(&kf) == dev3);
        kf.mFeatVec = full;
        orbm_keyframe* rebuilt = cache.Get(&kf);
        int n2 = 0, nodes2 = 0;
        OK(orbm_keyframe_fetch(ex, rebuilt, &n2, &nodes2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        EXPECT(cache.size() == 1 && n2 == N && nodes2 == nodes);
        std::vector<uint32_t> fnode2(nodes2); std::vector<int> nof(N), nof2(N);
        OK(orbm_keyframe_fetch(ex, rebuilt, nullptr, nullptr, nullptr, nullptr, nullptr, fnode2.data(), nullptr, nullptr, nof2.data()));
        OK(orbm_keyframe_fetch(ex, dev4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nof.data()));
        EXPECT(fnode2 == fnode && nof2 == nof);                    // what Get uploads of the host object is what the device made of the frame
        const long long live1 = device_allocations();
        EXPECT(cache.Get(&kf) == rebuilt && device_allocations() == live1);
    }
    {
        // the calling thread's cache, which the reference's own signatures use
        ORB_SLAM3::ORBmatcher::AdoptImplicit(&kf, dev4);
        const long long live0 = device_allocations();
        EXPECT(ORB_SLAM3::ORBmatcher::ImplicitCache<MockKeyFrame>().Get(&kf) == dev4 && device_allocations() == live0);
        ORB_SLAM3::ORBmatcher::EraseImplicit(&kf);
        EXPECT(ORB_SLAM3::ORBmatcher::ImplicitCache<MockKeyFrame>().size() == 0 && device_allocations() == live0 - 1);
    }
    orbv_destroy(voc);
    orbx_destroy(ex);
    if (failures) return 1;
    printf("ADOPT OK\n");
    return 0;
}
