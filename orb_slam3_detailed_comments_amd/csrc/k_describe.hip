// k_describe.hip — per-keypoint kernels of the ORB extractor:
//   k_layout        final output index of every keypoint: level scaling + lapping-area front/back
//                   reorder of ORBextractor::operator() (src/ORBextractor.cc:1613-1681) as prefix sums
//   k_orient_brief  a wave64 works through 8 keypoints: IC_Angle (:91-138, :580-591) on the raw level, then the
//                   256-bit steered BRIEF (:150-203) on the blurred level; 64 lanes x 4 rounds of
//                   __ballot assemble the four 64-bit descriptor words directly; the atan2 / cos / sin of
//                   the 8 keypoints are evaluated together, one keypoint per lane.
#include "orbx_types.h"
#include "orbx_block.h"
#include "orbx_simd.h"
#include "orbx_kernels.h"
#include "undistort_model.h"
#include "glibc_sincosf_model.h"
#include "glibc_logf_model.h"
#include "glibc_tanf_model.h"
#include "glibc_atan2f_model.h"

namespace orbx {

// rBRIEF pattern (data table of the reference, src/ORBextractor.cc:206-464), read through the scalar/L1 path
__device__ const signed char d_brief_pattern[1024] = {
#include "brief_pattern.inc"
};
#define BRIEF_PATTERN d_brief_pattern

// cv::fastAtan2 (OpenCV core mathfuncs): fp32, explicit IEEE ops, no contraction.
__device__ __forceinline__ float fast_atan2_deg(float y, float x) {
    const float s = (float)(180.0 / 3.1415926535897932384626433832795);
    const float p1 = 0.9997878412794807f * s, p3 = -0.3258083974640975f * s;
    const float p5 = 0.1555786518463281f * s, p7 = -0.04432655554792128f * s;
    const float eps = 2.2204460492503131e-16f;
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = __fdiv_rn(ay, __fadd_rn(ax, eps)); c2 = __fmul_rn(c, c);
        a = __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c);
    } else {
        c = __fdiv_rn(ax, __fadd_rn(ay, eps)); c2 = __fmul_rn(c, c);
        a = __fsub_rn(90.f, __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c));
    }
    if (x < 0) a = __fsub_rn(180.f, a);
    if (y < 0) a = __fsub_rn(360.f, a);
    return a;
}

// The steering of a keypoint from its patch moments (IC_Angle :91-138, computeOrbDescriptor :155-157): the angle in degrees, and the cos / sin of
// angle * factorPI that rotate the BRIEF pattern.  One definition for k_orient_brief and for k_model_selftest (op 7), which compares the
// composition with cv::fastAtan2 and the live cosf / sinf.
__device__ __forceinline__ void steer_from_moments(float m01, float m10, float* angle, float* a, float* b) {
    const float ang = fast_atan2_deg(m01, m10);
    const float factorPI = (float)(3.1415926535897932384626433832795 / 180.f);
    const float rad = __fmul_rn(ang, factorPI);
    *angle = ang; *a = glibc_cosf(rad); *b = glibc_sinf(rad);
}

// grid (B), 256 threads.  The level-ordered keypoint slots of an image (level l owns [kp_off, kp_off + kp_cap), the first lvl_count of them
// are in use) are walked in slot order = output order of the reference: a thread takes kLayoutPer consecutive slots, so that one workgroup
// scan per 256 * kLayoutPer slots (one in all for the usual feature counts) places every keypoint, with all key loads in flight at once.
constexpr int kLayoutPer = 8;
__global__ void __launch_bounds__(256) k_layout(const LevelInfo* __restrict__ lv, int nlevels,
                                                const uint32_t* __restrict__ lvl_keys, int kp_total_cap,
                                                const int* __restrict__ lvl_count, int lap0, int lap1,
                                                int* __restrict__ final_idx, int* __restrict__ n_out, int* __restrict__ mono_out,
                                                int nb, int* __restrict__ row_start, int* __restrict__ row_pos) {
    ORBX_DYN_SMEM(smem);                                // row index: histogram and cursors, (nb + 1) ints each
    __shared__ unsigned long long s_scan[20];
    __shared__ int s_cnt[kMaxLevels], s_off[kMaxLevels + 1];
    __shared__ float s_scale[kMaxLevels];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (tid < nlevels) { s_cnt[tid] = lvl_count[(size_t)b * nlevels + tid]; s_off[tid] = lv[tid].kp_off; s_scale[tid] = lv[tid].scale; }
    if (tid == 0) s_off[nlevels] = kp_total_cap;
    int* hist = (int*)smem; int* cursor = hist + (nb + 1);
    if (row_start != nullptr) for (int i = tid; i <= nb; i += 256) hist[i] = 0;
    __syncthreads();
    // bucket of the stereo row index (below): first row of the keypoint's candidate band
    auto bucket_of = [&](uint32_t key, int l) {
        float yf = (float)(key_y(key) + kBorder);
        if (l != 0) yf = __fmul_rn(yf, s_scale[l]);
        const int first = (int)floorf(__fsub_rn(yf, __fmul_rn(2.0f, s_scale[l])));     // = aux.x of k_orient_brief
        return imin(imax(first, 0) >> kStereoRowShift, nb - 1);
    };
    int total = 0;
    for (int l = 0; l < nlevels; l++) total += s_cnt[l];
    int mono_run = 0, lap_run = 0;
    // (declared outside the loop: with the usual feature counts the loop runs once and the row index below places the keypoints from these
    // registers instead of reading keys and output indices back)
    int valid[kLayoutPer], lvl[kLayoutPer], fin[kLayoutPer];
    uint32_t key[kLayoutPer];
    for (int base = 0; base < kp_total_cap; base += 256 * kLayoutPer) {
        const int s0 = base + tid * kLayoutPer;
        int l = 0;
        while (l + 1 < nlevels && s_off[l + 1] <= s0) l++;
#pragma unroll
        for (int k = 0; k < kLayoutPer; k++) {
            const int s = s0 + k;
            while (l + 1 < nlevels && s_off[l + 1] <= s) l++;
            lvl[k] = l;
            valid[k] = s < kp_total_cap && s - s_off[l] < s_cnt[l];
            key[k] = valid[k] ? lvl_keys[(size_t)b * kp_total_cap + s] : 0u;
        }
        int lapf[kLayoutPer], nm = 0, nl = 0;
#pragma unroll
        for (int k = 0; k < kLayoutPer; k++) {
            float xf = (float)(key_x(key[k]) + kBorder);
            if (lvl[k] != 0) xf = __fmul_rn(xf, s_scale[lvl[k]]);
            lapf[k] = valid[k] && xf >= (float)lap0 && xf <= (float)lap1;
            nm += valid[k] && !lapf[k]; nl += lapf[k];
            if (row_start != nullptr && valid[k]) atomicAdd(&hist[bucket_of(key[k], lvl[k])], 1);
        }
        unsigned long long tot;
        const unsigned long long ex = block_excl_scan<unsigned long long>((unsigned long long)nm | ((unsigned long long)nl << 32), &tot, s_scan);
        int pm = mono_run + (int)(ex & 0xFFFFFFFFu), pl = lap_run + (int)(ex >> 32);
#pragma unroll
        for (int k = 0; k < kLayoutPer; k++) {
            fin[k] = lapf[k] ? total - 1 - pl : pm;
            if (valid[k]) { final_idx[(size_t)b * kp_total_cap + s0 + k] = fin[k]; if (lapf[k]) pl++; else pm++; }
            // an unused slot is given one of the rows [total, cap) - the i-th unused slot row total + i - which k_orient_brief clears: descriptor
            // rows beyond the count read as zero (fixed-shape blocks for collectives) without a fill launch in front of every extraction
            else if (s0 + k < kp_total_cap) final_idx[(size_t)b * kp_total_cap + s0 + k] = total + (s0 + k) - (pm + pl);
        }
        mono_run += (int)(tot & 0xFFFFFFFFu); lap_run += (int)(tot >> 32);
    }
    if (tid == 0) { n_out[b] = total; mono_out[b] = mono_run; }
    // ---- row index for the stereo search (the role of vRowIndices, src/Frame.cc:1129-1155) ----
    // The keypoints of this image bucketed by the first row of their candidate band [floor(y - r), ceil(y + r)], r = 2 * scale
    // (1 << kStereoRowShift rows per bucket, CSR).  A left keypoint at row v then only visits the buckets that can
    // hold bands covering v.  Order inside a bucket is arbitrary (atomics): the search reduces full (distance << 16 | index) keys, so the
    // visiting order never shows in the result.  The band only needs the key and the level, so it is built here, where both are at hand,
    // instead of by a launch of its own in front of the match (a launch is 4.5 us of a single pair's latency).
    // What is stored is each slot's place in the bucket order, row_pos[slot]: k_orient_brief writes the slot's search record there, so that
    // the matcher reads the records of a run of buckets as one contiguous array (no index list between the buckets and the records).
    if (row_start == nullptr) return;
    __syncthreads();                                     // the histogram (counted in the loop above) is complete
    int run = 0;
    for (int c0 = 0; c0 < nb; c0 += 256) {
        const int c = c0 + tid;
        const int v = c < nb ? hist[c] : 0;
        unsigned long long tot;
        const int ex = run + (int)block_excl_scan<unsigned long long>((unsigned long long)v, &tot, s_scan);
        if (c < nb) { cursor[c] = ex; row_start[(size_t)b * (nb + 1) + c] = ex; }
        run += (int)tot;
    }
    if (tid == 0) row_start[(size_t)b * (nb + 1) + nb] = run;
    __syncthreads();
    if (kp_total_cap <= 256 * kLayoutPer) {             // one trip of the loop above: keys, levels and output indices are still in registers
#pragma unroll
        for (int k = 0; k < kLayoutPer; k++)
            if (valid[k]) row_pos[(size_t)b * kp_total_cap + tid * kLayoutPer + k] = atomicAdd(&cursor[bucket_of(key[k], lvl[k])], 1);
        return;
    }
    int l = 0;
    for (int s = tid; s < kp_total_cap; s += 256) {
        while (l + 1 < nlevels && s_off[l + 1] <= s) l++;
        if (s - s_off[l] < s_cnt[l])
            row_pos[(size_t)b * kp_total_cap + s] = atomicAdd(&cursor[bucket_of(lvl_keys[(size_t)b * kp_total_cap + s], l)], 1);
    }
}

// grid (groups_per_image * 8 * ceil(B / 8)) with groups_per_image = ceil(kp_total_cap / (4 * kKpPerWave)), 256 threads; a wave owns kKpPerWave
// consecutive keypoint slots.
//   1  one round trip fetches what the wave needs to begin: lane l the layout and count of level l, lane k the key, output index and bucket place
//      of keypoint k, every lane its disc half-widths and BRIEF tests; the wave then walks its valid keypoints, the patch loads of kPatchGroup
//      of them in flight together: IC_Angle moments with all 64 lanes (8 rows x 8 dword columns per trip, 4 trips), the sums go to lane k
//   2  the per-keypoint transcendental work - fastAtan2 and the fp64 cosf/sinf model - runs once for the whole wave, one keypoint
//      per lane, instead of 64-fold redundantly per keypoint (the first keypoint's window is already requested)
//   3  lane k writes the records of keypoint k
//   4  steered BRIEF, again one keypoint at a time with all lanes (4 tests per lane, 4 ballots = 4 descriptor words), the next keypoint's window
//      in flight while this one is sampled
constexpr int kKpPerWave = 8;                       // large batches; small ones use kKpPerWaveSmall (more, shorter waves: latency)
// window of the steered-BRIEF samples: rows / columns -18 .. +18 (the pattern's radius is 18.4), 10 dwords per row
constexpr int kWinR = 18, kWinRows = 2 * kWinR + 1, kWinDw = 10, kWinTrips = (kWinRows * kWinDw + 63) / 64;
static_assert(kKpPerWave == kKpPerWaveDecl, "orbx_kernels.h out of date");
constexpr int kKpPerWaveSmall = kKpPerWaveSmallDecl;
constexpr int kPatchGroup = 4;                      // IC_Angle: keypoints whose patches are in flight together (4 registers each)
// the register budget of both kernels: 8 waves per SIMD (64 registers), which is what hides the latency that is left
#ifdef ORBX_EMU
#define ORBX_EIGHT_WAVES
#else
#define ORBX_EIGHT_WAVES __attribute__((amdgpu_waves_per_eu(8, 8)))
#endif
template <int KPW>
__device__ __forceinline__ void orient_brief_impl(const LevelInfo* __restrict__ lv, int nlevels,
                                                      const uint8_t* __restrict__ pyr, const uint8_t* __restrict__ blur, size_t pyr_stride,
                                                      const uint32_t* __restrict__ lvl_keys, int kp_total_cap,
                                                      const int* __restrict__ lvl_count, const int* __restrict__ final_idx, const int* __restrict__ row_pos,
                                                      UmaxTab umax, KeyPointRec* __restrict__ out_kps,
                                                      unsigned long long* __restrict__ out_desc, int4* __restrict__ out_aux, int B, int groups_per_image) {
    __shared__ __attribute__((aligned(16))) uint8_t s_win[4][kWinRows * kWinDw * 4];
    // Workgroup -> (image, slot group).  Consecutive workgroup ids go to different XCDs (id % 8), each with its own L2; the keypoints of an
    // image read overlapping windows of the same pyramid / blur levels, so all workgroups of an image are kept on one XCD: groups of 8 images,
    // image = 8 * group + id % 8.  (With the plain (slot group, image) grid every XCD fetched every image: 470 MB per 128 images against 205 MB
    // of windows.)
    const int id = (int)blockIdx.x, nx = groups_per_image;
    const int b = 8 * (id / (8 * nx)) + (id & 7), gx = (id >> 3) % nx;
    if (b >= B) return;
    const int lane = lane_id();
    const int slot0 = (gx * 4 + (int)(threadIdx.x >> 6)) * KPW;
    if (slot0 >= kp_total_cap) return;
    // ---- 1a: every load whose address no loaded value decides goes out in one round trip ----
    // Lane l < nlevels fetches level l's layout and this image's count of it (the other lanes repeat the top level), a keypoint lane the key,
    // the output index and the bucket place of its slot (lanes >= KPW mirror lane 0 and are never read) - used or not: what an unused slot
    // holds is masked below - and every lane its disc half-widths and its four BRIEF tests.
    const int myslot = slot0 + (lane < KPW ? lane : 0);
    const int in_cap = myslot < kp_total_cap;
    const int ll = lane < nlevels ? lane : nlevels - 1;
    const int lv_kpoff = lv[ll].kp_off, lv_pitch = lv[ll].pitch, lv_off = lv[ll].off, lv_patch = lv[ll].patch;
    const float lv_scale = lv[ll].scale;
    const int lv_cnt = lvl_count[(size_t)b * nlevels + ll];
    const size_t sl = (size_t)b * kp_total_cap + (in_cap ? myslot : slot0);
    const uint32_t ld_key = lvl_keys[sl];
    const int my_fi = final_idx[sl], my_pos = row_pos[sl];
    // IC_Angle reads the 31 x 31 patch as dwords: lane = (row r8 = lane >> 3, column group c = lane & 7) covers columns u = -15 + 4c .. +3 of
    // rows v = -15 + 8 * trip + r8, four trips (the 32nd row / column carries weight 0), i.e. 4 load instructions per keypoint instead
    // of 16 byte gathers.  A lane's four rows have one half-width each: clamped index, the weight is masked afterwards.
    const int r8 = lane >> 3, cg = lane & 7;
    int um[4];
#pragma unroll
    for (int trip = 0; trip < 4; trip++) {
        const int v = -kHalfPatch + 8 * trip + r8;
        const int av = v < 0 ? -v : v;
        um[trip] = umax.u[av <= kHalfPatch ? av : 0];
    }
    // this lane's 4 tests (8 pattern points), the same for every keypoint: one dword each, unpacked when phase 3 begins
    uint32_t pat[4];
#pragma unroll
    for (int r = 0; r < 4; r++) pat[r] = load_u32_any((const uint8_t*)&BRIEF_PATTERN[4 * (64 * r + lane)]);
    // level of the slot: kp_off ascends, so it is the number of levels >= 1 that begin at or before the slot
    int my_level = 0;
    for (int l = 1; l < nlevels; l++) my_level += ORBX_READLANE(lv_kpoff, l) <= myslot;
    const int my_pitch = __shfl(lv_pitch, my_level), my_patch = __shfl(lv_patch, my_level);
    const float my_scale = __shfl(lv_scale, my_level);
    const int my_kpoff = __shfl(lv_kpoff, my_level), my_cnt = __shfl(lv_cnt, my_level);     // (every lane takes part: no `&&` in front of a shuffle)
    const int my_valid = in_cap && myslot - my_kpoff < my_cnt;
    if (!my_valid && in_cap && lane < KPW) {                // unused slot: clear the descriptor row k_layout assigned to it
        unsigned long long* z = out_desc + ((size_t)b * kp_total_cap + my_fi) * 4;
        z[0] = 0ull; z[1] = 0ull; z[2] = 0ull; z[3] = 0ull;
    }
    const uint32_t my_key = my_valid ? ld_key : 0u;
    // byte offset of the keypoint centre inside the image's pyramid / blur block (< 2^31)
    const int my_off = __shfl(lv_off, my_level) + (key_y(my_key) + kBorder) * my_pitch + (key_x(my_key) + kBorder);
    const unsigned long long vmask = __ballot(my_valid && lane < KPW);
    if (vmask == 0ull) return;
    const BufRsrc raw0 = buf_make(pyr + (size_t)b * pyr_stride);
    const BufRsrc blur0 = buf_make(blur + (size_t)b * pyr_stride);
    // ---- 1b: IC_Angle ----
    // The column moment is a v_dot4_u32_u8 per trip on unsigned weights: with u' = u + 16 inside the disc and 0 outside, sum(u * I) =
    // dot(I, u') - 16 * dot(I, on).  The four bytes of a trip lie in one row v, so the row moment is v * dot(I, on).  Integer sums: the
    // order of accumulation is irrelevant.
    uint32_t wu4[4], on4[4];
#pragma unroll
    for (int trip = 0; trip < 4; trip++) {
        const int v = -kHalfPatch + 8 * trip + r8;
        const int av = v < 0 ? -v : v;
        uint32_t pu = 0, po = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int u = -kHalfPatch + 4 * cg + j;
            const int au = u < 0 ? -u : u;
            const bool on = av <= kHalfPatch && au <= kHalfPatch && au <= um[trip];
            if (on) { pu |= (uint32_t)(u + 16) << (8 * j); po |= 1u << (8 * j); }
        }
        wu4[trip] = pu; on4[trip] = po;
    }
    // The wave walks its valid keypoints (the set bits of vmask, all wave-uniform) kPatchGroup at a time: the patch loads of a group go out
    // together and the keypoints are then reduced one after the other - two round trips for eight keypoints.  Only valid keypoints address the
    // image: a group that runs out of them repeats its last one, loads and sums (the same values into the same lane; a branch around the
    // repeat would let the compiler sink the loads behind it, and a wave is short of keypoints only where a level ends).
    auto patch_load = [&](int k, uint32_t (&I4)[4]) {
        const int pitch = ORBX_READLANE(my_pitch, k);
        // scalar offset of the trip's first row / column + per-lane (row, dword) offset: buffer addressing, no 64-bit vector arithmetic, and
        // one vector register of addresses per keypoint whatever the number of trips
        const uint32_t so = (uint32_t)(ORBX_READLANE(my_off, k) - kHalfPatch * pitch - kHalfPatch);
        const uint32_t vo = (uint32_t)(__mul24(r8, pitch) + 4 * cg);
#pragma unroll
        for (int trip = 0; trip < 4; trip++)                // issued back to back: one memory round trip
            I4[trip] = buf_load_u32(raw0, vo, so + (uint32_t)(8 * trip * pitch));
    };
    int my_m10 = 0, my_m01 = 0;
    auto patch_moments = [&](int k, const uint32_t (&I4)[4]) {
        uint32_t du = 0;
        int ds = 0, m01 = 0;
#pragma unroll
        for (int trip = 0; trip < 4; trip++) {
            const int s = (int)dot4_u8(I4[trip], on4[trip], 0u);
            du = dot4_u8(I4[trip], wu4[trip], du); ds += s; m01 += mul24(-kHalfPatch + 8 * trip + r8, s);
        }
        int m10 = (int)du - 16 * ds;
        m10 = wave_sum(m10); m01 = wave_sum(m01);
        if (lane == k) { my_m10 = m10; my_m01 = m01; }
    };
    const int kfirst = __ffsll(vmask) - 1;
    {
        constexpr int G = KPW < kPatchGroup ? KPW : kPatchGroup;
        unsigned long long rem = vmask;
        while (rem) {
            int ks[G];
            uint32_t I4[G][4];
#pragma unroll
            for (int g = 0; g < G; g++) {
                if (g == 0 || rem) { ks[g] = __ffsll(rem) - 1; rem &= rem - 1ull; }
                else ks[g] = ks[g - 1];
                patch_load(ks[g], I4[g]);
            }
#pragma unroll
            for (int g = 0; g < G; g++) patch_moments(ks[g], I4[g]);
        }
    }
    // ---- 4a: the first keypoint's window is requested before the steering math: its address does not depend on the angle ----
    // The 512 sample points of a keypoint fall inside the 37 x 37 window around it (pattern radius 18.4).  The wave copies that
    // window into its LDS slice with six row-coalesced dword loads per lane-trip (lanes of a row read 40 contiguous bytes) and then picks
    // the samples out of LDS: 512 scattered single-byte gathers from global memory per keypoint were what kept the texture path busy.
    uint8_t* win = s_win[threadIdx.x >> 6];
    auto win_load = [&](int k, uint32_t (&wv)[kWinTrips]) {
        const int pitch = ORBX_READLANE(my_pitch, k);
        const uint32_t so = (uint32_t)(ORBX_READLANE(my_off, k) - kWinR * pitch - kWinR);      // first row / column of the window
#pragma unroll
        for (int t = 0; t < kWinTrips; t++) {
            const int i = lane + 64 * t;                    // dword i of the window: row i / 10, dword column i % 10
            if (i < kWinRows * kWinDw) wv[t] = buf_load_u32(blur0, (uint32_t)(__mul24(i / kWinDw, pitch) + 4 * (i % kWinDw)), so);
        }
    };
    auto win_store = [&](const uint32_t (&wv)[kWinTrips]) {
        ORBX_WAVE_SYNC();                                   // the previous keypoint's samples have been read
#pragma unroll
        for (int t = 0; t < kWinTrips; t++) { const int i = lane + 64 * t; if (i < kWinRows * kWinDw) ((uint32_t*)win)[i] = wv[t]; }
        ORBX_WAVE_SYNC();
    };
    uint32_t wfirst[kWinTrips];
    win_load(kfirst, wfirst);
    // ---- 2: angle, cos, sin: one keypoint per lane ----
    float my_angle, my_a, my_b;
    steer_from_moments((float)my_m01, (float)my_m10, &my_angle, &my_a, &my_b);
    // ---- 3: records (before the descriptors: what only they need is dead from here on) ----
    if (lane < KPW && my_valid) {
        KeyPointRec k;
        float xf = (float)(key_x(my_key) + kBorder), yf = (float)(key_y(my_key) + kBorder);
        if (my_level != 0) { xf = __fmul_rn(xf, my_scale); yf = __fmul_rn(yf, my_scale); }
        k.x = xf; k.y = yf; k.size = (float)my_patch; k.angle = my_angle; k.response = (float)key_s(my_key);
        k.octave = my_level; k.class_id = -1;
        out_kps[(size_t)b * kp_total_cap + my_fi] = k;
        // compact 16-byte record for the stereo row search (Frame::ComputeStereoMatches, src/Frame.cc:1141-1155): the band of
        // image rows [floor(y - r), ceil(y + r)], r = 2 * scale, in which this keypoint is a candidate; x; octave and output index.
        // It goes to the keypoint's place in the bucket order of k_layout: the matcher reads a run of buckets as one array.
        const float r = __fmul_rn(2.0f, my_scale);
        int4 aux; aux.x = (int)floorf(__fsub_rn(yf, r)); aux.y = (int)ceilf(__fadd_rn(yf, r)); aux.z = __float_as_int(xf); aux.w = my_level | (my_fi << kAuxIndexShift);
        out_aux[(size_t)b * kp_total_cap + my_pos] = aux;
    }
    // ---- 4: steered BRIEF on the blurred level ----
    float px0[4], py0[4], px1[4], py1[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        px0[r] = (float)(signed char)(pat[r] & 0xFFu); py0[r] = (float)(signed char)((pat[r] >> 8) & 0xFFu);
        px1[r] = (float)(signed char)((pat[r] >> 16) & 0xFFu); py1[r] = (float)(signed char)(pat[r] >> 24);
    }
    // keypoint k's 256 tests on the window in LDS: 4 tests per lane, 4 ballots = 4 descriptor words
    auto brief = [&](int k) {
        const float a = __int_as_float(ORBX_READLANE(__float_as_int(my_a), k)), bb = __int_as_float(ORBX_READLANE(__float_as_int(my_b), k));
        const int fi = ORBX_READLANE(my_fi, k);
        // cvRound(x) for |x| < 2^22: x + 1.5 * 2^23 is rounded (to nearest, ties to even) at integer granularity, and its bit pattern is
        // 0x4B400000 + round(x).  The low 24 bits (0x400000 + r) feed the 24-bit multiply by the row pitch directly; all the constants are
        // folded into one subtraction per sample: offset = 40 * (r + 18) + (c + 18).
        constexpr float kRoundMagic = 12582912.0f;
        constexpr uint32_t kRoundFold = 0x400000u * (4u * kWinDw) + 0x4B400000u - (uint32_t)(kWinR * 4 * kWinDw + kWinR);
        int t0v[4], t1v[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint32_t r0 = __float_as_uint(__fadd_rn(__fadd_rn(__fmul_rn(px0[r], bb), __fmul_rn(py0[r], a)), kRoundMagic));
            const uint32_t c0 = __float_as_uint(__fadd_rn(__fsub_rn(__fmul_rn(px0[r], a), __fmul_rn(py0[r], bb)), kRoundMagic));
            const uint32_t r1 = __float_as_uint(__fadd_rn(__fadd_rn(__fmul_rn(px1[r], bb), __fmul_rn(py1[r], a)), kRoundMagic));
            const uint32_t c1 = __float_as_uint(__fadd_rn(__fsub_rn(__fmul_rn(px1[r], a), __fmul_rn(py1[r], bb)), kRoundMagic));
            t0v[r] = win[(uint32_t)__umul24(r0, 4 * kWinDw) + c0 - kRoundFold];
            t1v[r] = win[(uint32_t)__umul24(r1, 4 * kWinDw) + c1 - kRoundFold];
        }
        unsigned long long mine = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const unsigned long long w = ORBX_BALLOT(t0v[r] < t1v[r]);
            if (lane == r) mine = w;
        }
        if (lane < 4) out_desc[((size_t)b * kp_total_cap + fi) * 4 + lane] = mine;
    };
    // The six window loads of the next keypoint are in flight while this one is sampled out of LDS.  One LDS slice per wave: this keypoint's
    // samples are read, then (win_store's barrier) the next window is written.
    win_store(wfirst);
    {
        unsigned long long rem = vmask & (vmask - 1ull);
        int k = kfirst;
        while (rem) {
            const int kn = __ffsll(rem) - 1;
            rem &= rem - 1ull;
            uint32_t wn[kWinTrips];
            win_load(kn, wn);
            brief(k);
            win_store(wn);
            k = kn;
        }
        brief(k);
    }
}

__global__ void __launch_bounds__(256) ORBX_EIGHT_WAVES k_orient_brief(const LevelInfo* __restrict__ lv, int nlevels,
                                                      const uint8_t* __restrict__ pyr, const uint8_t* __restrict__ blur, size_t pyr_stride,
                                                      const uint32_t* __restrict__ lvl_keys, int kp_total_cap,
                                                      const int* __restrict__ lvl_count, const int* __restrict__ final_idx, const int* __restrict__ row_pos,
                                                      UmaxTab umax, KeyPointRec* __restrict__ out_kps,
                                                      unsigned long long* __restrict__ out_desc, int4* __restrict__ out_aux, int B, int groups_per_image) {
    orient_brief_impl<kKpPerWave>(lv, nlevels, pyr, blur, pyr_stride, lvl_keys, kp_total_cap, lvl_count, final_idx, row_pos, umax, out_kps, out_desc, out_aux, B, groups_per_image);
}
// the same with fewer keypoints per wave: four times as many, shorter waves (small batches, where one wave's chain of keypoints is the stage time)
__global__ void __launch_bounds__(256) ORBX_EIGHT_WAVES k_orient_brief_small(const LevelInfo* __restrict__ lv, int nlevels,
                                                      const uint8_t* __restrict__ pyr, const uint8_t* __restrict__ blur, size_t pyr_stride,
                                                      const uint32_t* __restrict__ lvl_keys, int kp_total_cap,
                                                      const int* __restrict__ lvl_count, const int* __restrict__ final_idx, const int* __restrict__ row_pos,
                                                      UmaxTab umax, KeyPointRec* __restrict__ out_kps,
                                                      unsigned long long* __restrict__ out_desc, int4* __restrict__ out_aux, int B, int groups_per_image) {
    orient_brief_impl<kKpPerWaveSmall>(lv, nlevels, pyr, blur, pyr_stride, lvl_keys, kp_total_cap, lvl_count, final_idx, row_pos, umax, out_kps, out_desc, out_aux, B, groups_per_image);
}

// Frame::UndistortKeyPoints (src/Frame.cc:1003-1034) for the keypoints of a batch: the records of `kps` with x, y replaced by cv::undistortPoints'
// result (undistort_model.h), everything else copied.  grid (ceil(cap / 256), B).
__global__ void __launch_bounds__(256) k_undistort(const KeyPointRec* __restrict__ kps, const int* __restrict__ n_per_frame, int cap, UndistortParams U,
                                                   KeyPointRec* __restrict__ kps_un) {
    const size_t b = blockIdx.y;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= cap || i >= n_per_frame[b]) return;
    KeyPointRec k = kps[b * (size_t)cap + i];
    float x, y;
    undistort_point(U, k.x, k.y, &x, &y);
    k.x = x; k.y = y;
    kps_un[b * (size_t)cap + i] = k;
}

// Self-test of the bit-exact function models (orbx_debug_model_eval; tests/test_model_sweep.py compares every result with the live libm /
// cv::fastAtan2's definition): one thread per element, out[i] = op(x, y) with x = a[i] - or, without a, the float whose bit pattern is
// start_bits + i - and y = b[i].  ops: 0 glibc_cosf, 1 glibc_sinf, 2 glibc_logf_model<false>, 3 glibc_tanf_model, 4 glibc_atanf_model,
// 5 glibc_atan2f_model(x, y), 6 fast_atan2_deg(x, y), 7 steer_from_moments(m01 = x, m10 = y): out[i] = angle, out[n + i] = cos, out[2 n + i] = sin
// (kModelSelftestOps in all).  Compiled with the flags of every other kernel; this is an instantiation of its own of the inline functions, not the
// copy inlined into k_orient_brief, k_frustum or the Kannala-Brandt kernels (without fast-math flags IEEE fixes the arithmetic of both).
__global__ void __launch_bounds__(256) k_model_selftest(int op, uint32_t start_bits, const float* __restrict__ a, const float* __restrict__ b, int n,
                                                        float* __restrict__ out) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const float x = a != nullptr ? a[i] : at_float(start_bits + (uint32_t)i);
    const float y = b != nullptr ? b[i] : 0.0f;
    float r = 0.0f;
    switch (op) {
        case 0: r = glibc_cosf(x); break;
        case 1: r = glibc_sinf(x); break;
        case 2: r = glibc_logf_model<false>(x); break;
        case 3: r = glibc_tanf_model(x); break;
        case 4: r = glibc_atanf_model(x); break;
        case 5: r = glibc_atan2f_model(x, y); break;
        case 6: r = fast_atan2_deg(x, y); break;
        default: {
            float ca, sa;
            steer_from_moments(x, y, &r, &ca, &sa);
            out[(size_t)n + i] = ca; out[2 * (size_t)n + i] = sa;
        }
    }
    out[i] = r;
}

}  // namespace orbx
