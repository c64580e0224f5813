// facade_gates_test.cpp — the decisions of include/orb_slam3_amd/ORBmatcher.h that the reference has no counterpart for, on the mock types of fuse_many_test.cpp:
//   cache     ORBmatcher::ResidentKeyFrames: each field of the tag, the transient entry of a key frame without BoW, the change of device, Trim at the capacities
//             1, 8, 9 and 16 (which entries go, how many, and that a hit renews an entry's age), the implicit cache's capacity.  What is resident is read off the
//             device objects themselves (orbm_keyframe_fetch) and off the library's count of live allocations, as keyframe_adopt_probe.cpp does.
//   rig       Fuse(vpKFs, vpMapPoints, th) on key frames of one camera MIXED with key frames of a two-camera rig, against the loop of the reference's call site
//             (src/LocalMapping.cc:991-1001: Fuse(pKFi, pts, th); if (pKFi->NLeft != -1) Fuse(pKFi, pts, true);), with points listed twice in the set: a rig key
//             frame takes the single calls, the points whose descriptor its surgery changed are searched again for the batched key frames behind it.
//   small     the same call on a HAND-BUILT world: five key frames of eight key points, ten set entries; what every key frame holds afterwards and every count is
//             written at the check and required of the loop and of the one call
//   smallsim3 that world through Fuse(vpKFs, vScw, vpPoints, th, hook) with the hook of LoopClosing::SearchAndFuse: held points, counts and every vpReplacePoint written
//   smallproj that world through SearchByProjection(vpKFs, vScw, vpPoints, [vpPointsKFs,] vvpMatched, [vvpMatchedKF,] th): every vvpMatched / vvpMatchedKF written
//   rigsim3, sim3proj   the Sim3 forms on the random world of fuse_many_test.cpp, the one call against the loop: a second, broader comparison
// Every expectation is written at its check.  argv[1] = "cache" | "small" | "smallsim3" | "smallproj" | "rig" | "rigsim3" | "sim3proj".  Prints "GATES OK".
#define FUSE_MANY_TEST_NO_MAIN
#include "fuse_many_test.cpp"

namespace {

int failures = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)
#define OK(call) do { const int rc_ = (call); if (rc_ != ORBX_OK) { printf("line %d: %s -> %d (%s)\n", __LINE__, #call, rc_, orbx_last_error()); exit(2); } } while (0)

typedef ORB_SLAM3::ORBmatcher Matcher;
typedef Matcher::ResidentKeyFrames<MockKeyFrame> Cache;

long long live() { long long l[4]; OK(orbx_debug_live_resources(l)); return l[0]; }

// a key frame of n keypoints whose descriptor rows all hold `fill` (so that the cache's fingerprint does not depend on n), features spread over `nodes` vocabulary nodes
void make(MockKeyFrame& kf, long unsigned id, int n, int nodes, unsigned char fill) {
    kf.mnId = id; kf.N = n; kf.NLeft = -1; kf.mpCamera2 = nullptr;
    kf.mvKeysUn.clear(); kf.mFeatVec.clear(); kf.mvScaleFactors.clear(); kf.mvLevelSigma2.clear();
    for (int i = 0; i < n; i++) kf.mvKeysUn.push_back(cv::KeyPoint(20.0f + 7 * i, 30.0f + 3 * i, 31.0f, 10.0f * i, 50.0f, i % 3));
    kf.mvKeys = kf.mvKeysUn; kf.mvuRight.assign(n, -1.0f);
    kf.mDescriptors = cv::Mat(n, 32, CV_8UC1); memset(kf.mDescriptors.ptr(0), fill, (size_t)n * 32);
    for (int i = 0; i < n && nodes > 0; i++) kf.mFeatVec[(unsigned)(i % nodes)].push_back((unsigned)i);
    float s = 1.0f;
    for (int l = 0; l < 8; l++) { kf.mvScaleFactors.push_back(s); kf.mvLevelSigma2.push_back(s * s); s *= 1.2f; }
}
struct Resident { int N = 0, nodes = 0; std::vector<unsigned char> desc; };
Resident fetch(orbm_keyframe* dev) {
    Resident r;
    OK(orbm_keyframe_fetch(Matcher::SharedHandle(), dev, &r.N, &r.nodes, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    r.desc.resize((size_t)(r.N > 0 ? r.N : 1) * 32);
    OK(orbm_keyframe_fetch(Matcher::SharedHandle(), dev, nullptr, nullptr, nullptr, r.desc.data(), nullptr, nullptr, nullptr, nullptr, nullptr));
    return r;
}

void TagFields() {
    Cache cache; MockKeyFrame kf;
    make(kf, 7, 16, 2, 0x11);
    const long long base = live();
    orbm_keyframe* d = cache.Get(&kf);
    EXPECT(cache.size() == 1 && live() == base + 1);
    EXPECT(cache.Get(&kf) == d && live() == base + 1);                       // a hit: the same object, nothing made
    // mnId: another key frame at the same address (row 1 is none of the eight rows of the fingerprint: 0 2 4 6 8 10 12 15 of 16)
    kf.mnId = 8; memset(kf.mDescriptors.ptr(1), 0x22, 32);
    EXPECT(fetch(cache.Get(&kf)).desc[32] == 0x22 && cache.size() == 1 && live() == base + 1);
    // N: four keypoints more, in the nodes that are there; every row holds the same bytes, so id, nodes and fingerprint stay
    make(kf, 8, 16, 2, 0x11); cache.Get(&kf);
    make(kf, 8, 20, 2, 0x11);
    EXPECT(fetch(cache.Get(&kf)).N == 20 && cache.size() == 1 && live() == base + 1);
    // the size of mFeatVec: ComputeBoW ran again on the host object
    make(kf, 8, 20, 3, 0x11);
    EXPECT(fetch(cache.Get(&kf)).nodes == 3 && cache.size() == 1 && live() == base + 1);
    // the fingerprint: row 0 is one of its rows
    memset(kf.mDescriptors.ptr(0), 0x33, 32);
    EXPECT(fetch(cache.Get(&kf)).desc[0] == 0x33 && cache.size() == 1 && live() == base + 1);
    cache.Clear();
    EXPECT(cache.size() == 0 && live() == base);
}

// a key frame whose mFeatVec is still empty is uploaded for the call and not cached; the cache holds ONE such object, released by the next upload or by Clear
void Transient() {
    Cache cache; MockKeyFrame a, b, c;
    make(a, 1, 12, 0, 0x41); make(b, 2, 12, 0, 0x42); make(c, 3, 12, 2, 0x43);
    const long long base = live();
    EXPECT(fetch(cache.Get(&a)).nodes == 0);
    EXPECT(cache.size() == 0 && live() == base + 1);
    EXPECT(fetch(cache.Get(&b)).desc[0] == 0x42);
    EXPECT(cache.size() == 0 && live() == base + 1);                         // a's object went when b's was made
    cache.Get(&c);                                                            // a cached upload releases it too
    EXPECT(cache.size() == 1 && live() == base + 1);
    cache.Get(&a);
    EXPECT(cache.size() == 1 && live() == base + 2);
    make(a, 1, 12, 2, 0x41);                                                  // ComputeBoW has run: cached from now on
    EXPECT(fetch(cache.Get(&a)).nodes == 2 && cache.size() == 2 && live() == base + 2);
    cache.Clear();
    EXPECT(live() == base);
}

// Trim at capacity C with C + 1 entries: drop = 1 + C / 8 entries go, the oldest first; a hit renews an entry's age.  The key frames are entered from the highest
// address down, so that age order is the reverse of the map's (address) order
void TrimAt(int C, int expectDropped) {
    Cache cache; std::vector<MockKeyFrame> kfs(C + 1);
    for (int i = 0; i <= C; i++) make(kfs[i], 100 + i, 8, 1, (unsigned char)i);
    auto at = [&](int age) -> MockKeyFrame* { return &kfs[C - age]; };      // age 0 = entered first
    const long long base = live();
    cache.SetCapacity(C);
    for (int age = 0; age < C; age++) cache.Get(at(age));
    cache.Trim();
    EXPECT((int)cache.size() == C && live() == base + C);                    // exactly at the bound: nothing goes
    cache.Get(at(C));
    cache.Get(at(0));                                                        // the oldest entry is used again: now the youngest
    cache.Trim();
    EXPECT((int)cache.size() == C + 1 - expectDropped && live() == base + C + 1 - expectDropped);
    const size_t n = cache.size();
    cache.Get(at(0));
    EXPECT(cache.size() == n);                                               // still there
    for (int age = expectDropped + 1; age <= C; age++) { cache.Get(at(age)); EXPECT(cache.size() == n); }      // and every entry younger than the dropped ones
    for (int age = 1; age <= expectDropped; age++) { cache.Get(at(age)); EXPECT(cache.size() == n + age); }     // the dropped ones are uploaded again
    cache.Clear();
    EXPECT(live() == base);
}

void Capacities() {
    {
        Cache cache; std::vector<MockKeyFrame> kfs(3);                        // capacity 0 = no bound: Trim leaves everything
        for (int i = 0; i < 3; i++) { make(kfs[i], 200 + i, 8, 1, (unsigned char)i); cache.Get(&kfs[i]); }
        cache.Trim();
        EXPECT(cache.Capacity() == 0 && cache.size() == 3);
    }
    TrimAt(1, 1); TrimAt(8, 2); TrimAt(9, 2); TrimAt(16, 3);
    EXPECT(Matcher::ImplicitCache<MockKeyFrame>().Capacity() == (size_t)Matcher::kImplicitCacheEntries);
    Matcher::SetImplicitCapacity<MockKeyFrame>(0);                            // 0 would mean "no bound" to Trim and "not set" to ImplicitCache: it is 1
    EXPECT(Matcher::ImplicitCache<MockKeyFrame>().Capacity() == 1);
    Matcher::SetImplicitCapacity<MockKeyFrame>((size_t)Matcher::kImplicitCacheEntries);
}

// device objects belong to one GPU: the first Get after the thread has moved to another one drops everything cached for the previous one
void DeviceChange() {
    if (orbx_device_count() < 2) { printf("one device: the device change is not exercised\n"); return; }
    Cache cache; MockKeyFrame a, b;
    make(a, 1, 12, 2, 0x51); make(b, 2, 12, 2, 0x52);
    cache.Get(&a); cache.Get(&b);
    EXPECT(cache.size() == 2);
    Matcher::SetThreadDevice(1);
    cache.Get(&a);
    EXPECT(cache.size() == 1);
    Matcher::SetThreadDevice(0);
    cache.Get(&b);
    EXPECT(cache.size() == 1);
    cache.Clear();
}

// ---- Fuse(vpKFs, ..) over one-camera and rig key frames ----
// targets 1 and 3 become rigs whose two cameras share pose and model: the first half of the keypoints is camera 1's, the rest camera 2's
void make_rigs(World& W) {
    for (int k : {1, 3}) {
        MockKeyFrame* kf = W.targets[k];
        kf->NLeft = kf->N / 2; kf->mpCamera2 = &kf->cam;
        kf->mvKeys.assign(kf->mvKeysUn.begin(), kf->mvKeysUn.begin() + kf->NLeft);
        kf->mvKeysRight.assign(kf->mvKeysUn.begin() + kf->NLeft, kf->mvKeysUn.end());
        for (cv::KeyPoint& r : kf->mvKeysRight) r.pt.x += 40.0f;             // (camera 2's own pixels: what mvKeysUn says of these features is not what a rig search reads)
    }
    // points listed twice: every 16th place of the set repeats the point three places before it
    for (size_t i = 16; i < W.set.size(); i += 16) W.set[i] = W.set[i - 3];
    // every second point of the set is well observed (it survives a Replace: `keep` is the incoming point) and carries a descriptor 46 bits from the one it had, at the
    // edge of TH_LOW: some key frames take it, some do not - until a Replace in one of them, a RIG among them, gives it the descriptor of its observations, which every
    // key frame behind takes: the batched rows behind a rig have to be searched again for it
    std::mt19937 g(7); std::set<MockMapPoint*> done;
    for (size_t i = 0; i < W.set.size(); i += 2) {
        MockMapPoint* p = W.set[i];
        if (!p || p->bad || !done.insert(p).second) continue;
        p->nObs += 50;
        std::set<int> bits; while ((int)bits.size() < 46) bits.insert((int)(g() % 256));
        cv::Mat m = p->desc.clone();
        for (int bit : bits) m.ptr(0)[bit >> 3] ^= (unsigned char)(1 << (bit & 7));
        p->desc = m;
    }
    // bad points that still sit at their keypoints (a point is made bad before the key frames that hold it let go of it): every 5th point a target holds
    int n = 0;
    for (MockKeyFrame* kf : W.targets) for (MockMapPoint* p : kf->points) if (p && n++ % 5 == 0) p->bad = true;
}

int Rig(bool sim3) {
    World A, B;
    build(A, sim3 ? 93u : 92u, 4000); build(B, sim3 ? 93u : 92u, 5000);
    make_rigs(A); make_rigs(B);
    if (sim3) for (World* W : {&A, &B}) { std::vector<MockMapPoint*> s; for (MockMapPoint* p : W->set) if (p) s.push_back(p); W->set.swap(s); }      // (vpPoints holds no NULL entries)
    Matcher matcher(0.8f);
    const float th = sim3 ? 4.0f : 3.0f;
    const int Mset = (int)A.set.size();
    std::vector<MockSim3> vScw;
    for (MockKeyFrame* kf : A.targets) { const float s = 1.02f; vScw.push_back(MockSim3{kf->pose.R, V3(kf->pose.t(0) * s, kf->pose.t(1) * s, kf->pose.t(2) * s), s}); }
    auto hook = [](World& W) { return [&W](int, std::vector<MockMapPoint*>& rep) { for (size_t i = 0; i < rep.size(); i++) if (rep[i]) rep[i]->Replace(W.set[i]); }; };
    std::vector<int> countsA;
    for (size_t k = 0; k < A.targets.size(); k++) {
        MockKeyFrame* kf = A.targets[k];
        if (!sim3) {                                                           // the call site, word for word: `true` lands in th
            int n = matcher.Fuse(kf, A.set, th);
            if (kf->NLeft != -1) n += matcher.Fuse(kf, A.set, true);
            countsA.push_back(n);
        } else {                                                               // src/LoopClosing.cc:2712-2745
            std::vector<MockMapPoint*> rep(Mset, nullptr);
            countsA.push_back(matcher.Fuse(kf, vScw[k], A.set, th, rep));
            hook(A)((int)k, rep);
        }
    }
    const std::vector<int> countsB = sim3 ? matcher.Fuse(B.targets, vScw, B.set, th, hook(B)) : matcher.Fuse(B.targets, B.set, th);
    const std::string a = dump(A, countsA), b = dump(B, countsB);
    int fused = 0, inRigs = countsA[1] + countsA[3]; for (int c : countsA) fused += c;
    printf("%s: fused %d (%d in the two rigs), Replace calls %d, identical %d\n", sim3 ? "rig sim3" : "rig", fused, inRigs, A.replaces, (int)(a == b));
    if (a != b) {
        size_t i = 0; while (i < a.size() && i < b.size() && a[i] == b[i]) i++;
        const size_t from = a.rfind('\n', i) == std::string::npos ? 0 : a.rfind('\n', i) + 1;
        printf("first difference:\n  A: %s\n  B: %s\n", a.substr(from, a.find('\n', i) - from).c_str(), b.substr(from, b.find('\n', i) - from).c_str());
        return 1;
    }
    // camera 2's keypoints of a rig take no new point: the second pass of the call site searches camera 1 again (its `true` is th = 1), and the Sim3 overload
    // has no second camera at all
    if (!sim3) for (World* W : {&A, &B}) for (const std::string& l : W->log) {
        int kf = -1, p = -1, slot = -1;
        if (sscanf(l.c_str(), "AddMapPoint %d %d %d", &kf, &p, &slot) == 3 && (kf == 1 || kf == 3) && slot >= W->targets[kf]->NLeft) { printf("a point entered camera 2 of a rig: %s\n", l.c_str()); return 1; }
    }
    if (A.replaces < 20 || inRigs < 20 || fused < 150) { printf("the world does not test the rig route\n"); return 1; }
    return 0;
}

// ---- the hand-built world: four target key frames of eight keypoints on a lattice, one key frame outside the call, ten entries in the point set ----
// Every camera stands at the origin (fx = fy = 500, cx = 320, cy = 240); feature j is the pixel (60 + 70 j, 200) at depth 4, on level 1.  F(j) is the descriptor of
// feature j; near(j, k, from) flips k bits of it from bit `from` on, so two descriptors of one feature are as far apart as their flipped bits differ.
// T0, T2, T3 have one camera and take the batched route; T1 is a rig (keypoints 0-3 camera 1, 4-7 camera 2) and takes the single calls, twice (th, then `true` = 1).
struct Small {
    World W;
    MockMapPoint *s[8], *rb, *r1, *r2, *r3, *rb7;
    static cv::Mat F(int j) { std::mt19937 g(1000 + j); cv::Mat m(1, 32, CV_8UC1); for (int b = 0; b < 32; b++) m.ptr(0)[b] = (unsigned char)(g() & 255); return m; }
    static cv::Mat near(int j, int k, int from = 0) { cv::Mat m = F(j); for (int bit = from; bit < from + k; bit++) m.ptr(0)[bit >> 3] ^= (unsigned char)(1 << (bit & 7)); return m; }
    MockMapPoint* point(int j, const cv::Mat& desc, int nObs) {
        std::unique_ptr<MockMapPoint> p(new MockMapPoint());
        p->world = &W; p->id = (int)W.points.size();
        p->pos = V3((60.0f + 70.0f * j - 320.0f) / 500.0f * 4.0f, (200.0f - 240.0f) / 500.0f * 4.0f, 4.0f);
        const float d = std::sqrt(p->pos(0) * p->pos(0) + p->pos(1) * p->pos(1) + p->pos(2) * p->pos(2));
        p->normal = V3(p->pos(0) / d, p->pos(1) / d, p->pos(2) / d);
        p->mfMaxDistance = d * std::sqrt(1.2f); p->mfMinDistance = p->mfMaxDistance / std::pow(1.2f, 7.0f);       // PredictScale = ceil(0.5) = 1
        p->desc = desc.clone(); p->nObs = nObs;
        W.points.push_back(std::move(p));
        return W.points.back().get();
    }
    void hold(int k, int slot, MockMapPoint* p) { W.kfs[k]->points[slot] = p; p->obs[W.kfs[k].get()] = slot; }
    Small() {
        for (int k = 0; k < 5; k++) {
            std::unique_ptr<MockKeyFrame> kf(new MockKeyFrame());
            kf->world = &W; kf->mnId = 9000 + k; kf->cam = MockCamera{{500.0f, 500.0f, 320.0f, 240.0f}}; kf->fx = kf->fy = 500.0f; kf->cx = 320.0f; kf->cy = 240.0f;
            kf->mfGridElementWidthInv = 64.0f / 640.0f; kf->mfGridElementHeightInv = 48.0f / 480.0f; kf->mfLogScaleFactor = std::log(1.2f);
            float sc = 1.0f;
            for (int l = 0; l < 8; l++) { kf->mvScaleFactors.push_back(sc); kf->mvLevelSigma2.push_back(sc * sc); kf->mvInvLevelSigma2.push_back(1.0f / (sc * sc)); sc *= 1.2f; }
            kf->N = 8; kf->mDescriptors = cv::Mat(8, 32, CV_8UC1);
            for (int j = 0; j < 8; j++) {
                kf->mvKeysUn.push_back(cv::KeyPoint(60.0f + 70.0f * j, 200.0f, 31.0f, 0.0f, 50.0f, 1));
                memcpy(kf->mDescriptors.ptr(j), F(j).ptr(0), 32);
                kf->mFeatVec[(unsigned)(j % 3)].push_back((unsigned)j);
            }
            kf->mvKeys = kf->mvKeysUn; kf->mvuRight.assign(8, -1.0f); kf->points.assign(8, nullptr);
            W.kfs.push_back(std::move(kf));
            if (k < 4) W.targets.push_back(W.kfs.back().get());
        }
        auto row = [&](int k, int j, const cv::Mat& d) { memcpy(W.kfs[k]->mDescriptors.ptr(j), d.ptr(0), 32); };
        MockKeyFrame* T1 = W.targets[1];
        T1->NLeft = 4; T1->mpCamera2 = &T1->cam;
        T1->mvKeys.assign(T1->mvKeysUn.begin(), T1->mvKeysUn.begin() + 4); T1->mvKeysRight.assign(T1->mvKeysUn.begin() + 4, T1->mvKeysUn.end());
        for (cv::KeyPoint& r : T1->mvKeysRight) r.pt.y += 40.0f;                  // (camera 2's own pixels)
        // feature 0: T1 holds a BAD point at keypoint 0.  s[0] meets it in both passes of the call site: counted twice there, nothing changes
        s[0] = point(0, near(0, 2), 1); rb = point(0, F(0), 2); rb->bad = true; hold(1, 0, rb);
        // feature 1: s[1] is 60 bits from the feature: no key frame takes it - but T1's row is 40 bits from it (20 from the feature) and holds r1, which has fewer
        // observations: r1 is replaced by s[1], s[1] takes T1's row as its descriptor, and T2 and T3, BEHIND the rig, take it now
        s[1] = point(1, near(1, 60), 50); r1 = point(1, F(1), 1); hold(1, 1, r1); row(1, 1, near(1, 20));
        // feature 2: s[2] stands TWICE in the set.  T2 - behind the rig, so that nothing but the replay's own note sees the change - has a row 45 bits from it and holds
        // r2 (fewer observations): s[2] survives with T2's row as its descriptor.  T3's row is 30 bits from s[2]'s FIRST descriptor (the candidate of the first search,
        // at both places of the set) and 75 from the new one: T3 must not take it, at either place.  T0 and T1 have unrelated rows there
        s[2] = point(2, F(2), 50); r2 = point(2, F(2), 1); hold(2, 2, r2); row(2, 2, near(2, 45)); row(3, 2, near(2, 30, 200)); row(0, 2, F(10)); row(1, 2, F(9));
        // feature 3: T0 holds r3 with more observations: s[3] is replaced (bad) and its observation outside the call goes to r3; no key frame behind sees s[3]
        s[3] = point(3, near(3, 1), 1); hold(4, 3, s[3]); r3 = point(3, F(3), 3); hold(0, 3, r3);
        // feature 4: camera 2 of the rig never takes a point (the second pass is camera 1 again); 5: a bad point; 6: T2 holds s[6] already; 7: T2 holds a bad point
        s[4] = point(4, near(4, 1), 1); s[5] = point(5, near(5, 1), 1); s[5]->bad = true; s[6] = point(6, near(6, 1), 1); hold(2, 6, s[6]);
        s[7] = point(7, near(7, 1), 1); rb7 = point(7, F(7), 2); rb7->bad = true; hold(2, 7, rb7);
        W.set = {s[0], s[1], s[2], nullptr, s[3], s[2], s[4], s[5], s[6], s[7]};
    }
    int id(MockMapPoint* p) const { return p ? p->id : -1; }
};

int SmallWorld() {
    Small A, B;
    Matcher matcher(0.8f);
    std::vector<int> countsA;
    for (MockKeyFrame* kf : A.W.targets) {                                    // src/LocalMapping.cc:991-1001, word for word
        int n = matcher.Fuse(kf, A.W.set, 3.0f);
        if (kf->NLeft != -1) n += matcher.Fuse(kf, A.W.set, true);
        countsA.push_back(n);
    }
    const std::vector<int> countsB = matcher.Fuse(B.W.targets, B.W.set, 3.0f);
    int bad = 0;
    for (int side = 0; side < 2; side++) {
        Small& S = side ? B : A; const std::vector<int>& counts = side ? countsB : countsA; const char* who = side ? "the one call" : "the loop of single calls";
        auto S_ = [&](int i) { return S.id(S.s[i]); };
        // what every key frame holds afterwards, keypoint by keypoint, and the counts: written here
        const std::vector<std::vector<int> > held = {
            {S_(0), -1, -1, S.id(S.r3), S_(4), -1, S_(6), S_(7)},                // T0: s0, r3 stays, s4, s6, s7; s1 is 60 bits away
            {S.id(S.rb), S_(1), -1, -1, -1, -1, -1, -1},                         // T1: the bad point stays, s1 in r1's place; s3 is bad by now; camera 2 takes nothing
            {S_(0), S_(1), S_(2), -1, S_(4), -1, S_(6), S.id(S.rb7)},            // T2: s1 after the refresh; s2 in r2's place; s6 was there; the bad point stays
            {S_(0), S_(1), -1, -1, S_(4), -1, S_(6), S_(7)},                     // T3: s2's new descriptor is 75 bits away
            {-1, -1, -1, S.id(S.r3), -1, -1, -1, -1}};                           // outside the call: s3's observation went to r3
        const std::vector<int> expect = {5, 3, 5, 5};                            // T1: s0 twice (both passes meet the bad point), s1 once
        for (int k = 0; k < 5; k++) for (int j = 0; j < 8; j++) if (S.id(S.W.kfs[k]->points[j]) != held[k][j]) {
            printf("SMALL %s: key frame %d keypoint %d holds point %d, written %d\n", who, k, j, S.id(S.W.kfs[k]->points[j]), held[k][j]); bad++;
        }
        for (int k = 0; k < 4; k++) if (counts[k] != expect[k]) { printf("SMALL %s: key frame %d fused %d, written %d\n", who, k, counts[k], expect[k]); bad++; }
        const bool flags = S.s[3]->bad && S.r1->bad && S.r2->bad && !S.r3->bad && !S.s[1]->bad && !S.s[2]->bad && !S.s[0]->bad;
        if (!flags) { printf("SMALL %s: bad flags: s3 %d r1 %d r2 %d r3 %d s1 %d s2 %d s0 %d\n", who, S.s[3]->bad, S.r1->bad, S.r2->bad, S.r3->bad, S.s[1]->bad, S.s[2]->bad, S.s[0]->bad); bad++; }
        if (memcmp(S.s[1]->desc.ptr(0), Small::near(1, 20).ptr(0), 32) || memcmp(S.s[2]->desc.ptr(0), Small::near(2, 45).ptr(0), 32)) { printf("SMALL %s: s1 / s2 do not carry the rows of T1 / T2\n", who); bad++; }
    }
    if (dump(A.W, countsA) != dump(B.W, countsB)) { printf("SMALL: the logs of the two worlds differ\n"); bad++; }
    printf("small world: counts %d %d %d %d, Replace calls %d, failures %d\n", countsB[0], countsB[1], countsB[2], countsB[3], B.W.replaces, bad);
    return bad;
}

void Check(int& bad, const char* what, const char* who, int k, const std::vector<int>& got, const std::vector<int>& written) {
    if (got == written) return;
    printf("SMALL %s, %s, key frame %d: got", what, who, k); for (int x : got) printf(" %d", x);
    printf(", written"); for (int x : written) printf(" %d", x);
    printf("\n"); bad++;
}
const MockSim3 kTwice = {M3{{1, 0, 0, 0, 1, 0, 0, 0, 1}}, V3(0, 0, 0), 2.0f};      // Scw with scale 2 at the origin: its rigid part is the key frames' own pose

// The hand-built world through Fuse(vpKFs, vScw, vpPoints, th, hook), the hook being LoopClosing::SearchAndFuse's pRep->Replace(point): here a key point that holds a
// point only REPORTS it, and the set's point always survives.  The set: s0 s1 s2 s3 s2 s4 s5 s6 s7 (no NULL entries; s2 twice; s5 bad).  The rig T1 takes the single
// call, which reads mvKeysUn - all eight key points, camera 2's at the pixels mvKeysUn holds for them (the batched route would read mvKeysRight).
int SmallSim3() {
    Small A, B;
    Matcher matcher(0.8f);
    int bad = 0;
    for (int side = 0; side < 2; side++) {
        Small& S = side ? B : A; const char* who = side ? "the one call" : "the loop of single calls";
        S.W.set = {S.s[0], S.s[1], S.s[2], S.s[3], S.s[2], S.s[4], S.s[5], S.s[6], S.s[7]};
        const int M = (int)S.W.set.size();
        std::vector<std::vector<int> > reported(4);
        auto hook = [&](int k, std::vector<MockMapPoint*>& rep) { for (int i = 0; i < M; i++) { reported[k].push_back(S.id(rep[i])); if (rep[i]) rep[i]->Replace(S.W.set[i]); } };
        std::vector<int> counts;
        const std::vector<MockSim3> vScw(4, kTwice);
        if (!side) for (int k = 0; k < 4; k++) {                               // src/LoopClosing.cc:2712-2745
            std::vector<MockMapPoint*> rep(M, nullptr); MockSim3 Scw = kTwice;
            counts.push_back(matcher.Fuse(S.W.targets[k], Scw, S.W.set, 4.0f, rep));
            hook(k, rep);
        } else counts = matcher.Fuse(S.W.targets, vScw, S.W.set, 4.0f, hook);
        auto S_ = [&](int i) { return S.id(S.s[i]); };
        const int rb = S.id(S.rb), r1 = S.id(S.r1), r2 = S.id(S.r2), r3 = S.id(S.r3), rb7 = S.id(S.rb7);
        const std::vector<std::vector<int> > held = {
            {S_(0), -1, -1, S_(3), S_(4), -1, S_(6), S_(7)},                     // T0: r3 was reported and replaced by s3 in the hook; s1 is 60 bits away, s2's row is unrelated
            {rb, S_(1), -1, S_(3), S_(4), -1, S_(6), S_(7)},                     // T1, the rig: the bad point stays (counted, not reported); s1 in r1's place; camera 2's key points take s4, s6, s7
            {S_(0), S_(1), S_(2), S_(3), S_(4), -1, S_(6), rb7},                 // T2: s1 with the row it took in T1 (searched again); s2 in r2's place; s6 was there; the bad point stays
            {S_(0), S_(1), -1, S_(3), S_(4), -1, S_(6), S_(7)},                  // T3: s2 carries T2's row now, 75 bits from this one: the candidate of the first search is dropped
            {-1, -1, -1, S_(3), -1, -1, -1, -1}};                                // outside the call: s3 keeps its observation
        const std::vector<std::vector<int> > written = {                        // vpReplacePoint per key frame, by place in the set
            {-1, -1, -1, r3, -1, -1, -1, -1, -1},
            {-1, r1, -1, -1, -1, -1, -1, -1, -1},                                // not rb: a bad point at the key point is not reported (:1650)
            {-1, -1, r2, -1, r2, -1, -1, -1, -1},                                // s2 stands twice and meets r2 at both places; not rb7
            {-1, -1, -1, -1, -1, -1, -1, -1, -1}};
        const std::vector<int> expect = {5, 6, 7, 6};                            // T0: s0 s3 s4 s6 s7; T1: s0 s1 s3 s4 s6 s7; T2: s0 s1 s2 s2 s3 s4 s7 (s6 is held); T3: s0 s1 s3 s4 s6 s7
        for (int k = 0; k < 5; k++) { std::vector<int> got; for (int j = 0; j < 8; j++) got.push_back(S.id(S.W.kfs[k]->points[j])); Check(bad, "held", who, k, got, held[k]); }
        for (int k = 0; k < 4; k++) Check(bad, "vpReplacePoint", who, k, reported[k], written[k]);
        Check(bad, "counts", who, -1, counts, expect);
        if (!(S.r1->bad && S.r2->bad && S.r3->bad && !S.s[3]->bad && !S.s[1]->bad && !S.s[2]->bad)) { printf("SMALL sim3 %s: bad flags\n", who); bad++; }
        if (memcmp(S.s[1]->desc.ptr(0), Small::near(1, 20).ptr(0), 32) || memcmp(S.s[2]->desc.ptr(0), Small::near(2, 45).ptr(0), 32)) { printf("SMALL sim3 %s: s1 / s2 do not carry the rows of T1 / T2\n", who); bad++; }
    }
    printf("small world, Sim3 Fuse: failures %d\n", bad);
    return bad;
}

// The hand-built world through the Sim3 projection search.  The set: s0 s1 s2 s3 s4 s5 s6 s7 (s5 bad).  On entry key point 5 of T0 holds s4 and key point 0 of T2 holds
// s7: such a point takes no part for that key frame, and its key point is occupied.  Nothing is written into the key frames: the answer is vvpMatched (and vvpMatchedKF)
int SmallProjection(bool withKFs) {
    Small A, B;
    Matcher matcher(0.8f);
    int bad = 0;
    for (int side = 0; side < 2; side++) {
        Small& S = side ? B : A; const char* who = side ? "the one call" : "the loop of single calls";
        S.W.set = {S.s[0], S.s[1], S.s[2], S.s[3], S.s[4], S.s[5], S.s[6], S.s[7]};
        const int M = 8;
        std::vector<MockKeyFrame*> pointKFs(M);
        for (int i = 0; i < M; i++) pointKFs[i] = S.W.kfs[i % 5].get();          // point i came from key frame i % 5
        std::vector<std::vector<MockMapPoint*> > matched(4, std::vector<MockMapPoint*>(8, nullptr)); std::vector<std::vector<MockKeyFrame*> > matchedKF(4, std::vector<MockKeyFrame*>(8, nullptr));
        matched[0][5] = S.s[4]; matched[2][0] = S.s[7];
        const std::vector<MockSim3> vScw(4, kTwice);
        std::vector<int> counts;
        if (!side) for (int k = 0; k < 4; k++) { MockSim3 Scw = kTwice; counts.push_back(withKFs ? matcher.SearchByProjection(S.W.targets[k], Scw, S.W.set, pointKFs, matched[k], matchedKF[k], 3, 1.0f)
                                                                                                 : matcher.SearchByProjection(S.W.targets[k], Scw, S.W.set, matched[k], 3, 1.0f)); }
        else counts = withKFs ? matcher.SearchByProjection(S.W.targets, vScw, S.W.set, pointKFs, matched, matchedKF, 3, 1.0f) : matcher.SearchByProjection(S.W.targets, vScw, S.W.set, matched, 3, 1.0f);
        auto S_ = [&](int i) { return S.id(S.s[i]); };
        const std::vector<std::vector<int> > written = {
            {S_(0), -1, -1, S_(3), -1, S_(4), S_(6), S_(7)},                     // T0: s4 is held by key point 5 on entry: not searched, key point 4 stays free; s1 60 bits away; s2's row unrelated
            {S_(0), S_(1), -1, S_(3), S_(4), -1, S_(6), S_(7)},                  // T1, the rig, by the single call over mvKeysUn: s1 is 40 bits from its row; camera 2's key points take s4 s6 s7
            {S_(7), -1, S_(2), S_(3), S_(4), -1, S_(6), -1},                     // T2: key point 0 is occupied by s7 on entry: s0 finds nothing, and s7 is not searched; s2 is 45 bits from its row
            {S_(0), -1, S_(2), S_(3), S_(4), -1, S_(6), S_(7)}};                 // T3: s2 is 30 bits from its row
        // vvpMatchedKF: the key frame of the matched point (its place in the set % 5) at the key points matched by THIS call, nothing at the ones held on entry
        const std::vector<std::vector<int> > writtenKF = {{0, -1, -1, 3, -1, -1, 1, 2}, {0, 1, -1, 3, 4, -1, 1, 2}, {-1, -1, 2, 3, 4, -1, 1, -1}, {0, -1, 2, 3, 4, -1, 1, 2}};
        const std::vector<int> expect = {4, 6, 4, 6};
        for (int k = 0; k < 4; k++) {
            std::vector<int> got, gotKF;
            for (int j = 0; j < 8; j++) { got.push_back(S.id(matched[k][j])); gotKF.push_back(matchedKF[k][j] ? kf_index(matchedKF[k][j]) : -1); }
            Check(bad, "vvpMatched", who, k, got, written[k]);
            if (withKFs) Check(bad, "vvpMatchedKF", who, k, gotKF, writtenKF[k]);
        }
        Check(bad, "counts", who, -1, counts, expect);
    }
    printf("small world, Sim3 projection%s: failures %d\n", withKFs ? " with key frames" : "", bad);
    return bad;
}

// SearchByProjection(vpKFs, vScw, vpPoints, vvpMatched, th) - one point set searched from many key frames - against the single call per key frame: rigs among the key
// frames (they take the single call), and every 9th keypoint holds a point OF THE SET on entry (it is taken: occupied, and not searched again for that key frame)
int Sim3Projection(bool withKFs) {
    World A, B;
    build(A, 94u, 6000); build(B, 94u, 7000);
    make_rigs(A); make_rigs(B);
    for (World* W : {&A, &B}) { std::vector<MockMapPoint*> s; for (MockMapPoint* p : W->set) if (p) s.push_back(p); W->set.swap(s); }
    Matcher matcher(0.8f);
    const int th = 4, Mset = (int)A.set.size(), Kn = (int)A.targets.size();
    std::vector<MockSim3> vScw;
    for (MockKeyFrame* kf : A.targets) { const float s = 1.02f; vScw.push_back(MockSim3{kf->pose.R, V3(kf->pose.t(0) * s, kf->pose.t(1) * s, kf->pose.t(2) * s), s}); }
    auto index_of = [](World& W, MockMapPoint* p) { return p ? p->id : -1; };
    std::string out[2]; int total = 0, taken = 0;
    for (int side = 0; side < 2; side++) {
        World& W = side ? B : A;
        std::vector<std::vector<MockMapPoint*> > matched(Kn); std::vector<std::vector<MockKeyFrame*> > matchedKF(Kn);
        std::vector<MockKeyFrame*> pointKFs(Mset);
        for (int i = 0; i < Mset; i++) pointKFs[i] = W.kfs[i % W.kfs.size()].get();
        for (int k = 0; k < Kn; k++) {
            matched[k].assign(W.targets[k]->N, nullptr); matchedKF[k].assign(W.targets[k]->N, nullptr);
            for (int i = 0; i < W.targets[k]->N; i += 9) { matched[k][i] = W.set[(i * 7 + k) % Mset]; if (!side) taken++; }
        }
        std::vector<int> counts;
        if (!side) for (int k = 0; k < Kn; k++) counts.push_back(withKFs ? matcher.SearchByProjection(W.targets[k], vScw[k], W.set, pointKFs, matched[k], matchedKF[k], th, 1.0f)
                                                                         : matcher.SearchByProjection(W.targets[k], vScw[k], W.set, matched[k], th, 1.0f));
        else counts = withKFs ? matcher.SearchByProjection(W.targets, vScw, W.set, pointKFs, matched, matchedKF, th, 1.0f) : matcher.SearchByProjection(W.targets, vScw, W.set, matched, th, 1.0f);
        char b[48];
        for (int k = 0; k < Kn; k++) {
            snprintf(b, sizeof b, "count %d\n", counts[k]); out[side] += b; if (!side) total += counts[k];
            for (int i = 0; i < W.targets[k]->N; i++) { snprintf(b, sizeof b, " %d:%d", index_of(W, matched[k][i]), matchedKF[k][i] ? kf_index(matchedKF[k][i]) : -1); out[side] += b; }
            out[side] += "\n";
        }
    }
    printf("sim3 projection%s: %d matches, %d keypoints held a point of the set on entry, identical %d\n", withKFs ? " with key frames" : "", total, taken, (int)(out[0] == out[1]));
    if (out[0] != out[1]) return 1;
    if (total < 150 || taken < 60) { printf("the world does not test the search\n"); return 1; }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string what = argc > 1 ? argv[1] : "";
    if (what == "small") { if (SmallWorld()) return 1; }
    else if (what == "smallsim3") { if (SmallSim3()) return 1; }
    else if (what == "smallproj") { if (SmallProjection(false) || SmallProjection(true)) return 1; }
    else if (what == "rig") { if (Rig(false)) return 1; }
    else if (what == "rigsim3") { if (Rig(true)) return 1; }
    else if (what == "sim3proj") { if (Sim3Projection(false) || Sim3Projection(true)) return 1; }
    else if (what == "cache") {
        Matcher::SharedHandle();                                                 // (the thread's handle, before anything is counted)
        const long long base = live();
        TagFields(); Transient(); Capacities(); DeviceChange();
        Matcher::ClearImplicit<MockKeyFrame>();
        EXPECT(live() == base);
        if (failures) return 1;
    } else return 2;
    printf("GATES OK\n");
    return 0;
}
