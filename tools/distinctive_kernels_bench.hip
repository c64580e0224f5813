// HIP-event times of k_distinctive_resident (observations read from resident key frames, winners written to a store) and k_distinctive (the same rows
// gathered by the host beforehand) on the same map points.  tools/bench_distinctive_resident.py writes the points to a file, builds this program into
// tools/bin/ and runs it:   distinctive_kernels_bench <points file> <repetitions>
// File (int32 unless stated): nkf, P, total, sizes[nkf], descriptors of every key frame one behind the other (uint8 [sum sizes][32]), obs_start[P + 1],
// obs_kf[total], obs_feat[total].  Prints one JSON line: median / p10 / p90 in microseconds over the repetitions, the two kernels alternating.
#include "../orb_slam3_detailed_comments_amd/csrc/k_match.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace orbx;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <typename T> static T* upload(const std::vector<T>& v) {
    T* d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(v.size(), 1) * sizeof(T)) != hipSuccess) return nullptr;
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}
static void stats(std::vector<float> t, const char* name, bool last) {
    std::sort(t.begin(), t.end());
    const size_t n = t.size();
    printf("\"%s\": {\"us\": %.2f, \"p10\": %.2f, \"p90\": %.2f}%s", name, 1e3 * t[n / 2], 1e3 * t[n / 10], 1e3 * t[std::min(n - 1, n * 9 / 10)], last ? "" : ", ");
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s <points file> <repetitions>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    const int reps = atoi(argv[2]);
    int head[3];
    if (!f || fread(head, 4, 3, f) != 3 || reps < 1) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const int nkf = head[0], P = head[1], total = head[2];
    std::vector<int> sizes(nkf), start(P + 1), okf(total), ofeat(total);
    if (fread(sizes.data(), 4, nkf, f) != (size_t)nkf) return 2;
    size_t rows = 0;
    std::vector<size_t> first(nkf);
    for (int k = 0; k < nkf; k++) { first[k] = rows; rows += sizes[k]; }
    std::vector<unsigned long long> desc(4 * rows);
    if (fread(desc.data(), 32, rows, f) != rows || fread(start.data(), 4, P + 1, f) != (size_t)P + 1 || fread(okf.data(), 4, total, f) != (size_t)total ||
        fread(ofeat.data(), 4, total, f) != (size_t)total) return 2;
    fclose(f);
    // the resident side: one block of key-frame descriptors, the table of their starts, the launch lists (register form first) with a store row per point
    unsigned long long* d_kf = upload(desc);
    std::vector<const unsigned long long*> table(nkf);
    for (int k = 0; k < nkf; k++) table[k] = d_kf + 4 * first[k];
    unsigned long long* d_store = nullptr;
    CHECK(hipMalloc(&d_store, 32 * (size_t)std::max(P, 1)));
    std::vector<DistinctiveRec> recs; std::vector<int> point_of;
    int n_reg = 0, largest = 0;
    for (int form = 0; form < 2; form++) {
        for (int p = 0; p < P; p++) {
            const int n = start[p + 1] - start[p];
            if (n == 0 || n > kDistinctiveMax || (n > kDistinctiveRegMax) != (form == 1)) continue;
            recs.push_back({d_store + 4 * (size_t)p, start[p], n}); point_of.push_back(p); largest = std::max(largest, n);
        }
        if (form == 0) n_reg = (int)recs.size();
    }
    const int n_rec = (int)recs.size(), n_lds = n_rec - n_reg;
    // the gathered side: the rows of the observations, one behind the other
    std::vector<unsigned long long> rows_g(4 * (size_t)total);
    for (int o = 0; o < total; o++)
        for (int w = 0; w < 4; w++) rows_g[4 * (size_t)o + w] = desc[4 * (first[okf[o]] + ofeat[o]) + w];
    const unsigned long long* const* d_table = upload(table);
    const int *d_okf = upload(okf), *d_ofeat = upload(ofeat), *d_start = upload(start);
    const DistinctiveRec* d_recs = upload(recs);
    const unsigned long long* d_rows = upload(rows_g);
    int *d_best_r = nullptr, *d_best_g = nullptr; unsigned long long* d_best_desc = nullptr;
    CHECK(hipMalloc(&d_best_r, 4 * (size_t)std::max(n_rec, 1))); CHECK(hipMalloc(&d_best_g, 4 * (size_t)std::max(P, 1))); CHECK(hipMalloc(&d_best_desc, 32 * (size_t)std::max(n_rec, 1)));
    if (!d_kf || !d_table || !d_okf || !d_ofeat || !d_start || !d_recs || !d_rows) { fprintf(stderr, "allocation failed\n"); return 1; }
    hipStream_t s; CHECK(hipStreamCreate(&s));
    hipEvent_t e0, e1; CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    auto resident = [&]() {
        if (n_reg > 0) ORBX_LAUNCH(k_distinctive_resident<false>, dim3((n_reg + 3) / 4), dim3(256), 0, s, d_recs, 0, n_reg, d_table, d_okf, d_ofeat, d_best_r, d_best_desc);
        if (n_lds > 0) ORBX_LAUNCH(k_distinctive_resident<true>, dim3(n_lds), dim3(64), 32 * (size_t)largest, s, d_recs, n_reg, n_lds, d_table, d_okf, d_ofeat, d_best_r, d_best_desc);
    };
    auto gathered = [&]() { ORBX_LAUNCH(k_distinctive, dim3((P + 3) / 4), dim3(256), 0, s, d_rows, d_start, P, d_best_g); };
    std::vector<float> t_r, t_g;
    for (int it = -3; it < reps; it++) {                                         // three warm-up rounds
        float ms_r = 0, ms_g = 0;
        CHECK(hipEventRecord(e0, s)); resident(); CHECK(hipEventRecord(e1, s)); CHECK(hipEventSynchronize(e1)); CHECK(hipEventElapsedTime(&ms_r, e0, e1));
        CHECK(hipEventRecord(e0, s)); gathered(); CHECK(hipEventRecord(e1, s)); CHECK(hipEventSynchronize(e1)); CHECK(hipEventElapsedTime(&ms_g, e0, e1));
        CHECK(hipGetLastError());
        if (it >= 0) { t_r.push_back(ms_r); t_g.push_back(ms_g); }
    }
    // both kernels choose the same rows
    std::vector<int> best_r(std::max(n_rec, 1)), best_g(std::max(P, 1));
    CHECK(hipMemcpy(best_r.data(), d_best_r, 4 * (size_t)n_rec, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(best_g.data(), d_best_g, 4 * (size_t)P, hipMemcpyDeviceToHost));
    for (int r = 0; r < n_rec; r++)
        if (best_r[r] != best_g[point_of[r]]) { fprintf(stderr, "point %d: k_distinctive_resident keeps row %d, k_distinctive row %d\n", point_of[r], best_r[r], best_g[point_of[r]]); return 1; }
    printf("{\"points\": %d, \"observations\": %d, \"register_form_points\": %d, \"lds_form_points\": %d, \"largest\": %d, ", P, total, n_reg, n_lds, largest);
    stats(t_r, "k_distinctive_resident", false); stats(t_g, "k_distinctive", true);
    printf("}\n");
    return 0;
}
