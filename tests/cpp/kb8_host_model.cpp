// csrc/kb8_model.h compiled for the host (g++ -O2 -ffp-contract=off; tests/test_kb8_stereo_constructed.py): the expected values of k_kb8_stereo on injected keypoints.
#include "kb8_model.h"

extern "C" void kb8_unproject(const float* cam, const float* uv, int n, float* rays) {
    orbx::KB8Cam c;
    for (int k = 0; k < 8; k++) c.p[k] = cam[k];
    for (int i = 0; i < n; i++) orbx::kb8_unproject(c, uv[2 * i], uv[2 * i + 1], rays + 3 * i);
}

// z[i] = the return value of kb8_triangulate_matches (depth, or the rejection codes -1 .. -5), p3d[3 i ..] = the point where it accepts (0 otherwise)
extern "C" void kb8_triangulate_matches(const float* cam1, const float* cam2, const float* R12, const float* t12, const float* uv1, const float* uv2,
                                        const float* sigma1, const float* sigma2, int n, float* z, float* p3d) {
    orbx::KB8Cam c1, c2;
    for (int k = 0; k < 8; k++) { c1.p[k] = cam1[k]; c2.p[k] = cam2[k]; }
    for (int i = 0; i < n; i++) {
        float r1[3], r2[3], p[3] = {0.f, 0.f, 0.f};
        orbx::kb8_unproject(c1, uv1[2 * i], uv1[2 * i + 1], r1);
        orbx::kb8_unproject(c2, uv2[2 * i], uv2[2 * i + 1], r2);
        z[i] = orbx::kb8_triangulate_matches(c1, c2, r1, r2, uv1[2 * i], uv1[2 * i + 1], uv2[2 * i], uv2[2 * i + 1], R12, t12, sigma1[i], sigma2[i], p);
        p3d[3 * i] = p[0]; p3d[3 * i + 1] = p[1]; p3d[3 * i + 2] = p[2];
    }
}
