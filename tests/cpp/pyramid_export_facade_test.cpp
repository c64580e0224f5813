// The drop-in ORBextractor's mvImagePyramid after the device export (orbx_set_pyramid_export): over consecutive calls on one extractor each level
// is a view into the handle's export slot, its bytes - the 19-px border included - equal the former host path (orbx_pyramid_fetch of the levels, then
// cv::copyMakeBorder(BORDER_REFLECT_101 + BORDER_ISOLATED) around each), and the previous call's Mats are still intact.
//   pyramid_export_facade_test w h calls im0.raw [im1.raw ...]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ORBextractor.h"

static const int E = 19;
static std::vector<std::vector<unsigned char>> framed_bytes(const std::vector<cv::Mat>& pyr) {       // rows -19 .. rows + 18 of every level
    std::vector<std::vector<unsigned char>> out;
    for (const cv::Mat& m : pyr) {
        std::vector<unsigned char> v;
        for (int y = -E; y < m.rows + E; y++) { const unsigned char* r = m.data + (ptrdiff_t)y * (ptrdiff_t)m.step - E; v.insert(v.end(), r, r + m.cols + 2 * E); }
        out.push_back(v);
    }
    return out;
}

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: pyramid_export_facade_test w h calls im0.raw [im1.raw ...]\n"); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]), calls = atoi(argv[3]), nim = argc - 4;
    std::vector<std::vector<unsigned char>> ims(nim, std::vector<unsigned char>((size_t)w * h));
    for (int i = 0; i < nim; i++) {
        FILE* f = fopen(argv[4 + i], "rb");
        if (!f || fread(ims[i].data(), 1, ims[i].size(), f) != ims[i].size()) { fprintf(stderr, "read failed: %s\n", argv[4 + i]); return 3; }
        fclose(f);
    }
    ORB_SLAM3::ORBextractor ex(1000, 1.2f, 8, 20, 7);
    const int nl = ex.GetLevels();
    std::vector<cv::KeyPoint> kps; cv::Mat desc; std::vector<int> lap = {0, 0};
    std::vector<cv::Mat> prev_mats; std::vector<std::vector<unsigned char>> prev_bytes;
    int bad = 0;
    for (int c = 0; c < calls; c++) {
        cv::Mat im(h, w, CV_8UC1, ims[c % nim].data());
        ex(im, cv::Mat(), kps, desc, lap);
        // (1) the levels are views into the handle's export slot
        const uint8_t* base = nullptr; std::vector<size_t> off(nl); std::vector<int> step(nl), lw(nl), lh(nl);
        if (orbx_pyramid_exported(ex.Handle(), 0, &base, off.data(), step.data(), lw.data(), lh.data()) != ORBX_OK) { fprintf(stderr, "exported: %s\n", orbx_last_error()); return 4; }
        for (int l = 0; l < nl; l++) {
            const cv::Mat& m = ex.mvImagePyramid[l];
            if (m.data != base + off[l] + (size_t)E * step[l] + E || (int)m.step != step[l] || m.cols != lw[l] || m.rows != lh[l]) {
                fprintf(stderr, "call %d level %d: mvImagePyramid is not a view of the export slot\n", c, l); bad++;
            }
        }
        // (2) the former host path, restated: one fetch of the levels, copyMakeBorder around each
        std::vector<cv::Mat> framed(nl), lvl(nl); std::vector<uint8_t*> dst(nl); std::vector<int> stride(nl);
        for (int l = 0; l < nl; l++) {
            framed[l] = cv::Mat(cv::Size(lw[l] + 2 * E, lh[l] + 2 * E), CV_8UC1);
            lvl[l] = framed[l](cv::Rect(E, E, lw[l], lh[l]));
            dst[l] = lvl[l].data; stride[l] = (int)lvl[l].step;
        }
        if (orbx_pyramid_fetch(ex.Handle(), 0, 0, dst.data(), stride.data()) != ORBX_OK) { fprintf(stderr, "fetch: %s\n", orbx_last_error()); return 5; }
        for (int l = 0; l < nl; l++) cv::copyMakeBorder(lvl[l], framed[l], E, E, E, E, cv::BORDER_REFLECT_101 + cv::BORDER_ISOLATED);
        const std::vector<std::vector<unsigned char>> want = framed_bytes(lvl), got = framed_bytes(ex.mvImagePyramid);
        for (int l = 0; l < nl; l++) if (want[l] != got[l]) { fprintf(stderr, "call %d level %d: framed bytes differ from the host path\n", c, l); bad++; }
        // (3) what the previous call handed out is intact
        if (c > 0) {
            const std::vector<std::vector<unsigned char>> again = framed_bytes(prev_mats);
            for (int l = 0; l < nl; l++) if (again[l] != prev_bytes[l]) { fprintf(stderr, "call %d: the previous call's level %d changed\n", c, l); bad++; }
        }
        prev_mats = ex.mvImagePyramid; prev_bytes = got;
    }
    // SetExportPyramid(false): the call still extracts, and mvImagePyramid keeps the views it held (nothing is exported, nothing is asked for)
    {
        ex.SetExportPyramid(false);
        cv::Mat im(h, w, CV_8UC1, ims[0].data());
        std::vector<cv::KeyPoint> k2; cv::Mat d2;
        ex(im, cv::Mat(), k2, d2, lap);
        if (k2.empty() || d2.rows != (int)k2.size()) { fprintf(stderr, "no features without the export\n"); bad++; }
        for (int l = 0; l < nl; l++) if (ex.mvImagePyramid[l].data != prev_mats[l].data) { fprintf(stderr, "level %d changed with the export switched off\n", l); bad++; }
        ex.SetExportPyramid(true);
        ex(im, cv::Mat(), k2, d2, lap);
        const uint8_t* base = nullptr; std::vector<size_t> off(nl); std::vector<int> step(nl), lw(nl), lh(nl);
        if (orbx_pyramid_exported(ex.Handle(), 0, &base, off.data(), step.data(), lw.data(), lh.data()) != ORBX_OK) { fprintf(stderr, "exported: %s\n", orbx_last_error()); return 4; }
        for (int l = 0; l < nl; l++) if (ex.mvImagePyramid[l].data != base + off[l] + (size_t)E * step[l] + E) { fprintf(stderr, "level %d is no view of the export slot after switching it on again\n", l); bad++; }
        // an empty image: -1, as the reference (src/ORBextractor.cc:1089-1090)
        if (ex(cv::Mat(), cv::Mat(), k2, d2, lap) != -1) { fprintf(stderr, "an empty image did not return -1\n"); bad++; }
    }
    printf("%s: %d calls, %d mismatches\n", bad ? "FAIL" : "ok", calls, bad);
    return bad ? 1 : 0;
}
