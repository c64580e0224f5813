// Threaded comparer of tests/test_model_sweep.py (g++ -O2 -ffp-contract=off -shared -fPIC -I csrc -lpthread): the results of orbx_debug_model_eval against
// what the host computes - the LIVE libm for ops 0 .. 5 (cosf, sinf, logf, tanf, atanf, atan2f), cv::fastAtan2 as the oracle restates it
// (oracle/orb_primitives.h, the definition behind orbo_fast_atan2) for op 6, and both composed as the reference composes them (src/ORBextractor.cc:155-157)
// for op 7.  Equal means equal bit patterns, or NaN on both sides.  host_model evaluates the csrc model headers compiled for the host at single inputs, so a
// failure can say which of device build, host build and libm stands alone.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../oracle/orb_primitives.h"
#include "glibc_sincosf_model.h"
#include "glibc_logf_model.h"
#include "glibc_tanf_model.h"
#include "glibc_atan2f_model.h"

namespace {

inline uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
inline float float_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
inline bool same(float a, float b) { return bits_of(a) == bits_of(b) || (a != a && b != b); }

// the expected value(s) of an op: r[0], and r[1], r[2] for op 7
template <int OP>
inline void expect(float x, float y, float* r) {
    if (OP == 0) r[0] = cosf(x);
    else if (OP == 1) r[0] = sinf(x);
    else if (OP == 2) r[0] = logf(x);
    else if (OP == 3) r[0] = tanf(x);
    else if (OP == 4) r[0] = atanf(x);
    else if (OP == 5) r[0] = atan2f(x, y);
    else if (OP == 6) r[0] = orbp::fast_atan2_deg(x, y);
    else {
        const float factorPI = (float)(3.1415926535897932384626433832795 / 180.f);
        r[0] = orbp::fast_atan2_deg(x, y);                      // IC_Angle: fastAtan2((float)m_01, (float)m_10)
        const float rad = r[0] * factorPI;                      // float angle = (float)kpt.angle * factorPI
        r[1] = cosf(rad); r[2] = sinf(rad);                     // (float)cos(angle), (float)sin(angle) of a float: cosf / sinf
    }
}

template <int OP>
void compare_range(uint32_t start_bits, const float* a, const float* b, long long n, const float* dev, long long lo, long long hi, long long* bad, long long* first) {
    long long nb = 0, fb = -1;
    for (long long i = lo; i < hi; i++) {
        const float x = a ? a[i] : float_of(start_bits + (uint32_t)i), y = b ? b[i] : 0.0f;
        float r[3];
        expect<OP>(x, y, r);
        bool ok = same(r[0], dev[i]);
        if (OP == 7) ok = ok && same(r[1], dev[n + i]) && same(r[2], dev[2 * n + i]);
        if (!ok) { if (fb < 0) fb = i; nb++; }
    }
    *bad = nb; *first = fb;
}

typedef void (*range_fn)(uint32_t, const float*, const float*, long long, const float*, long long, long long, long long*, long long*);
const range_fn kRange[8] = {compare_range<0>, compare_range<1>, compare_range<2>, compare_range<3>, compare_range<4>, compare_range<5>, compare_range<6>, compare_range<7>};

}  // namespace

// number of elements i in [0, n) whose device result (dev_out[i]; for op 7 also dev_out[n + i], dev_out[2 n + i]) differs from the host's expectation;
// *first_bad_index = the smallest such i, or -1.  -1 for an unknown op or missing operands.
extern "C" long long sweep_compare(int op, uint32_t start_bits, const float* a, const float* b, long long n, const float* dev_out, int threads, long long* first_bad_index) {
    if (op < 0 || op > 7 || n < 0 || !dev_out || !first_bad_index || (op >= 5 && (!a || !b))) return -1;
    if (threads < 1) threads = 1;
    if ((long long)threads > n) threads = n > 0 ? (int)n : 1;
    std::vector<long long> bad(threads, 0), first(threads, -1);
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back(kRange[op], start_bits, a, b, n, dev_out, n * t / threads, n * (t + 1) / threads, &bad[t], &first[t]);
    for (auto& th : pool) th.join();
    long long total = 0; *first_bad_index = -1;
    for (int t = 0; t < threads; t++) {
        total += bad[t];
        if (first[t] >= 0 && *first_bad_index < 0) *first_bad_index = first[t];       // the slices are in index order
    }
    return total;
}

// the host's expectation at one input: out[0] (out[0 .. 2] for op 7); returns the number of values written
extern "C" int host_expect(int op, float x, float y, float* out) {
    switch (op) {
        case 0: expect<0>(x, y, out); return 1;
        case 1: expect<1>(x, y, out); return 1;
        case 2: expect<2>(x, y, out); return 1;
        case 3: expect<3>(x, y, out); return 1;
        case 4: expect<4>(x, y, out); return 1;
        case 5: expect<5>(x, y, out); return 1;
        case 6: expect<6>(x, y, out); return 1;
        case 7: expect<7>(x, y, out); return 3;
    }
    return 0;
}

// the model headers of csrc compiled for the host, at one input.  fast_atan2_deg is a device function of k_describe.hip and has no host build of its own
// (the emulator library is its host build): op 6 writes nothing, op 7 takes the angle from cv::fastAtan2's definition and applies the header's cos / sin.
extern "C" int host_model(int op, float x, float y, float* out) {
    switch (op) {
        case 0: out[0] = orbx::glibc_cosf(x); return 1;
        case 1: out[0] = orbx::glibc_sinf(x); return 1;
        case 2: out[0] = orbx::glibc_logf_model<false>(x); return 1;
        case 3: out[0] = orbx::glibc_tanf_model(x); return 1;
        case 4: out[0] = orbx::glibc_atanf_model(x); return 1;
        case 5: out[0] = orbx::glibc_atan2f_model(x, y); return 1;
        case 7: {
            const float factorPI = (float)(3.1415926535897932384626433832795 / 180.f);
            out[0] = orbp::fast_atan2_deg(x, y);
            const float rad = out[0] * factorPI;
            out[1] = orbx::glibc_cosf(rad); out[2] = orbx::glibc_sinf(rad);
            return 3;
        }
    }
    return 0;
}

// out[i] = cv::fastAtan2(a[i], b[i]) as the oracle defines it (the test scans its pair grid for angles next to 0, 90, 180, 270 and 360 degrees)
extern "C" void fast_atan2_many(const float* a, const float* b, long long n, float* out, int threads) {
    if (threads < 1) threads = 1;
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back([=] { for (long long i = n * t / threads; i < n * (t + 1) / threads; i++) out[i] = orbp::fast_atan2_deg(a[i], b[i]); });
    for (auto& th : pool) th.join();
}
