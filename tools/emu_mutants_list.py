"""The mutants of tools/emu_mutants.py: (id, file in csrc - or, from the repository root, a header under include/orb_slam3_amd -, old text that occurs EXACTLY ONCE in that file, new text, CPU test files or node ids, intent[, note][, defines]).

Only decisions are mutated: a relational boundary, one clause of a compound gate removed or negated, a rank or threshold constant off by one, a tie broken the other
way, a gate's constant replaced by a neighbour.  Never address arithmetic, loop bounds over memory, launch geometry, synchronisation or the lines under the
debug_flags test switches: the emulator runs inside the test process, and a mutant must not be able to index outside its arrays.  That also keeps out the clauses
whose only purpose is to keep reads inside an array (`inb` of k_stereo_match, the `q < cap` tests) and the gates in front of a readlane / an index (`bestinc == -Lh`
may be moved inwards, not removed).

`note`: the reason why a mutant that survives is no gap in the suite - it computes the same on every input (equivalent), or no input that the library accepts reaches the
value where it differs.  A survivor without a note is a missing test.  Ids are stable: add at the end of a file's block, never renumber."""

STEREO = ["test_stereo_constructed_descriptors.py", "test_branch_edges_stereo.py", "test_stereo_ties.py", "test_stereo_chain.py", "test_match_empty_edges.py",
          "test_stereo_disparity_range.py"]
KNN = ["test_knn2_constructed.py", "test_match_empty_edges.py", "test_kb8_stereo_constructed.py", "test_kb8.py"]
KB8 = ["test_kb8_stereo_constructed.py", "test_kb8.py", "test_match_empty_edges.py"]
DISTINCTIVE = ["test_distinctive_resident.py", "test_emu_mappoint.py"]

MUTANTS = []


def M(id, file, old, new, tests, intent, note=None, more=(), defines=()):
    """more: further (old, new) pairs of the same mutant, each old text unique too - for a decision that is written at two places (a tie order packed into a key and unpacked again)
    defines: compiler switches the mutant's whole library is built with (the variants of tests/test_emu_variants.py), for decisions the default build reaches only on huge inputs
    tests: file names, or pytest node ids where the whole file takes minutes on the emulator; cheapest first"""
    MUTANTS.append(dict(id=id, file=file, old=old, new=new, tests=list(tests), intent=intent, note=note, more=list(more), defines=list(defines)))


# ---- k_match.hip ---------------------------------------------------------------------------------------------------------------------------------------------
F = "k_match.hip"
DELTA = ("equivalent: bestinc is the FIRST minimum of the eleven SADs and not at either end, so dist1 > dist2 <= dist3 and |dist1 - dist3| <= dist1 + dist3 - 2 dist2, "
         "i.e. |deltaR| <= 0.5 (integers below 2^15: every operation before the division is exact); the gate is never entered (tests/test_branch_edges_stereo.py asserts the bound)")
# k_stereo_match: gate
M(1, F, "return rowL >= a.x &&", "return rowL > a.x &&", STEREO, "stereo gate: first row of the band exclusive")
M(2, F, "&& rowL <= a.y &&", "&& rowL < a.y &&", STEREO, "stereo gate: last row of the band exclusive")
M(3, F, "oct >= levelL - 1 &&", "oct > levelL - 1 &&", STEREO, "stereo gate: the octave below refused")
M(4, F, "oct <= levelL + 1 &&", "oct < levelL + 1 &&", STEREO, "stereo gate: the octave above refused")
M(5, F, "xr >= minU && xr <= maxU;", "xr > minU && xr <= maxU;", STEREO, "stereo gate: x == minU refused")
M(6, F, "xr >= minU && xr <= maxU;", "xr >= minU && xr < maxU;", STEREO, "stereo gate: x == maxU refused")
M(7, F, "oct >= levelL - 1 && oct <= levelL + 1 && ", "", STEREO, "stereo gate: the octave clause removed")
# :120
M(8, F, "bestDist < P.th_orb && nr > 0", "bestDist <= P.th_orb && nr > 0", STEREO, "stereo: distance th_orb goes on to the refinement")
M(9, F, "bestDist < P.th_orb && nr > 0", "bestDist < P.th_orb", STEREO, "stereo: the nr > 0 clause removed",
  "equivalent: without right keypoints every bucket is empty (jbeg == jend), best stays TH_HIGH << 16 and bestDist = TH_HIGH is not below th_orb")
M(10, F, "P.th_high << 16;", "(P.th_high + 1) << 16;", STEREO, "stereo: a candidate at TH_HIGH replaces the start value",
   "equivalent in the output: a winner at distance TH_HIGH is not below th_orb and ends as -1 like no winner.  Precondition th_orb <= th_high: both are set in one place, "
   "orbm_stereo_match (csrc/orbx_api.cpp: P.th_high = 100, P.th_orb = (100 + 50) / 2, ORBmatcher::TH_HIGH / TH_LOW), and no entry point takes either")
# :130
M(11, F, "endu >= (float)Lw", "endu > (float)Lw", STEREO, "stereo: endu == level width accepted",
   "unreachable: endu == Lw needs a right keypoint whose x, rounded at the LEFT keypoint's level, is Lw - 11.  orbm_stereo_match reads the right keypoints' x only from "
   "the search records that the right extraction wrote (d_aux: no entry point returns or takes its address, tests/resident_inject.py), and the extractor keeps a keypoint "
   "of level m at x <= w_m - 17 of its level; with |m - levelL| <= 1 that is at most Lw - 17 / 1.2 + rounding = Lw - 13 at the left keypoint's level.  "
   "The reference's answer at the boundary is pinned on the oracle by tests/test_stereo_disparity_range.py::test_oracle_window_guard_at_the_level_border")
M(12, F, "!(iniu < 0 ||", "!(iniu <= 0 ||", STEREO, "stereo: iniu == 0 refused",
   "equivalent: iniu == 0 means cr == 0, and the `inb` clause cr - Lh - w >= 0 already refuses it")
# :160 - :168
M(13, F, "bestinc == -Lh ||", "bestinc == -Lh + 1 ||", STEREO, "stereo: the second shift counts as the window's end")
M(14, F, "|| bestinc == Lh))", "|| bestinc == Lh - 1))", STEREO, "stereo: the last shift but one counts as the window's end")
M(15, F, "deltaR < -1 ||", "deltaR <= -1 ||", STEREO, "stereo: deltaR == -1 refused", DELTA)
M(16, F, "|| deltaR > 1))", "|| deltaR >= 1))", STEREO, "stereo: deltaR == 1 refused", DELTA)
M(17, F, "disparity >= 0 && disparity < maxD", "disparity > 0 && disparity < maxD", STEREO, "stereo: disparity 0 refused instead of clamped")
M(18, F, "disparity >= 0 && disparity < maxD", "disparity >= 0 && disparity <= maxD", STEREO, "stereo: disparity == maxD accepted")
M(19, F, "if (disparity <= 0) {", "if (disparity < 0) {", STEREO, "stereo: disparity 0 not clamped to 0.01")
M(20, F, "disparity >= 0 && disparity < maxD", "disparity < maxD", STEREO, "stereo: the disparity >= 0 clause removed")
# k_stereo_median
M(21, F, "if (!((float)s < thDist))", "if ((float)s > thDist)", STEREO, "median: SAD == thDist kept")
M(22, F, "pass ? s_med[2] : cnt / 2;", "pass ? s_med[2] : (cnt - 1) / 2;", STEREO, "median: rank (cnt - 1) / 2")
M(23, F, "if (s >= 0) {", "if (s > 0) {", STEREO, "median: a match with SAD 0 neither kept nor erased")
M(24, F, "if (s >= 0 && (pass == 0", "if (s > 0 && (pass == 0", STEREO, "median: SAD 0 left out of the median")
M(25, F, "1.5f * 1.4f", "1.5f * 1.5f", STEREO, "median: factor 2.25 instead of 2.1")
# k_knn2 / k_knn2_mfma
M(26, F, "\n        ratio_ok[o] = (i1 >= 0 && (double)(float)dd0 < ", "\n        ratio_ok[o] = (i1 >= 0 && (double)(float)dd0 <= ", KNN, "knn2: ratio test inclusive")
M(27, F, "\n            ratio_ok[o] = (i1 >= 0 && (double)(float)dd0 < ", "\n            ratio_ok[o] = (i1 >= 0 && (double)(float)dd0 <= ", KNN, "knn2_mfma: ratio test inclusive")
M(28, F, "\n        ratio_ok[o] = (i1 >= 0 && ", "\n        ratio_ok[o] = (", KNN, "knn2: a query without second neighbour passes the ratio test")
M(29, F, "\n            ratio_ok[o] = (i1 >= 0 && ", "\n            ratio_ok[o] = (", KNN, "knn2_mfma: a query without second neighbour passes the ratio test")
M(30, F, "(int)(b0 >> 16), dd1 = i1 < 0 ?", "(int)(b0 >> 16), dd1 = i1 <= 0 ?", KNN, "knn2: second neighbour 0 reported without distance")
M(31, F, "(int)(k0 >> 16), dd1 = i1 < 0 ?", "(int)(k0 >> 16), dd1 = i1 <= 0 ?", KNN, "knn2_mfma: second neighbour 0 reported without distance")
M(32, F, "if ((int)(key & 0xFFFFu) >= nT) key", "if ((int)(key & 0xFFFFu) > nT) key", KNN, "knn2_mfma: the row behind the train set is a neighbour")
# (ids 33 and 34, `q >= nQ` -> `q > nQ` in k_knn2 and k_knn2_mfma, are not in the list: the mutant reads - k_knn2 - or writes - both - the row behind the query set, which lies
# inside the arrays only because they are sized to the capacity.  The line is covered from the other side: tests/test_match_empty_edges.py checks the -1 rows behind the set.)
M(35, F, "if (k0 == b0) k0 = k1;", "if (k0 != b0) k0 = k1;", KNN, "knn2: the runner-up exposed by the wrong lanes")
# k_kb8_stereo
M(36, F, "if (z > 0.0001f) {", "if (z > 0.0f) {", KB8, "kb8 stereo: depth gate 0 instead of 1e-4")
M(37, F, "if (z > 0.0001f) {", "if (z >= 0.0001f) {", KB8, "kb8 stereo: depth gate inclusive")
M(38, F, "i < nL[b] && q >= 0 && ratio_ok", "i < nL[b] && q > 0 && ratio_ok", KB8, "kb8 stereo: the first lapping keypoint left out")
M(39, F, "atomicMax(&r2l[", "atomicMin(&r2l[", KB8, "kb8 stereo: the smallest left index wins mvRightToLeftMatch")
# k_distinctive, distinctive_point
M(40, F, "const int rank = (N - 1) >> 1;", "const int rank = N >> 1;", DISTINCTIVE, "distinctive: rank N / 2")
M(41, F, "if (median < bestMedian) {", "if (median <= bestMedian) {", DISTINCTIVE, "distinctive: the last of equal medians wins")
M(42, F, "median < 0 && rank < before + c[t]", "median < 0 && rank <= before + c[t]", DISTINCTIVE, "distinctive: the bin before the rank's")
M(43, F, "N = R.n, rank = (N - 1) >> 1;", "N = R.n, rank = N >> 1;", DISTINCTIVE, "distinctive (resident): rank N / 2")
M(44, F, "if (count_le(bestMedian - 1) > rank) {", "if (count_le(bestMedian) > rank) {", DISTINCTIVE, "distinctive (resident): the last of equal medians wins")
M(45, F, "if (count_le(mid) > rank) hi = mid;", "if (count_le(mid) >= rank) hi = mid;", DISTINCTIVE, "distinctive (resident): bisection one rank low")
M(46, F, "ORBX_BALLOT(d[c] <= v)", "ORBX_BALLOT(d[c] < v)", DISTINCTIVE, "distinctive (resident): count of distances below v, not up to v",
  note="equivalent: with `<` the bisection returns median + 1 for every row and the winner test `count(bestMedian - 1) > rank` becomes median_i < median_best again - bestMedian is off by one consistently and never leaves the function (a median of 256, which the start value 257 would not admit, loses to no row and leaves bestIdx = 0 as the reference does)")

# ---- k_search.hip --------------------------------------------------------------------------------------------------------------------------------------------
F = "k_search.hip"
LOCAL = ["test_branch_edges_search.py", "test_emu_search.py", "test_local_points.py", "test_local_points_batch.py", "test_local_points_maps.py", "test_local_map_search.py",
         "test_search_gates.py"]
PROJ = ["test_lastframe_batch.py", "test_keyframe_batch.py", "test_map_rows_projection.py", "test_branch_edges_rotation.py", "test_emu_search.py", "test_branch_edges_search.py",
        "test_search_gates.py", "test_lastframe_gates.py"]
RIG = ["test_rig_tracking_batch.py", "test_local_points_rig.py", "test_rig_local_points_maps.py", "test_search_gates.py"]
FUSE = ["test_fuse_batch.py", "test_fuse_map.py", "test_emu_search.py", "test_search_gates.py", "test_projection_gates.py"]
SIM3 = ["test_sim3_projection_batch.py", "test_sim3_map.py", "test_emu_search.py", "test_search_gates.py"]
BOW = ["test_branch_edges_triangulation.py", "test_emu_search.py", "test_bow_frames_batch.py", "test_map_rows_bow.py", "test_branch_edges_rotation.py", "test_rig_bow_batch.py",
       "test_keyframe_search_gates.py"]
MAP = ["test_map_rows_resident.py", "test_map_rows_bow.py", "test_map_rows_projection.py", "test_local_map_build.py", "test_fuse_map.py", "test_sim3_map.py", "test_local_map_search.py",
       "test_map_state_gates.py"]
# area_accept
M(100, F, "if (k.octave < A.min_level) return false;", "if (k.octave <= A.min_level) return false;", LOCAL + PROJ[:2], "area: the lowest level of the window refused")
M(101, F, "A.max_level >= 0 && k.octave > A.max_level", "A.max_level >= 0 && k.octave >= A.max_level", LOCAL + PROJ[:2], "area: the highest level of the window refused")
M(102, F, "if (A.max_level >= 0 && k.octave", "if (A.max_level > 0 && k.octave", LOCAL + PROJ[:2], "area: max level 0 means no upper limit")
M(103, F, "fabsf(__fsub_rn(k.x, A.x)) < A.r &&", "fabsf(__fsub_rn(k.x, A.x)) <= A.r &&", LOCAL, "area: |dx| == r inside the box")
M(104, F, "fabsf(__fsub_rn(k.y, A.y)) < A.r))", "fabsf(__fsub_rn(k.y, A.y)) <= A.r))", LOCAL, "area: |dy| == r inside the box")
M(105, F, "if (ur > 0 && fabsf(__fsub_rn(A.ur, ur)) > A.r)", "if (ur >= 0 && fabsf(__fsub_rn(A.ur, ur)) > A.r)", LOCAL + PROJ[:1], "area: a right coordinate of exactly 0 is gated")
M(106, F, "if (ur > 0 && fabsf(__fsub_rn(A.ur, ur)) > A.r)", "if (ur > 0 && fabsf(__fsub_rn(A.ur, ur)) >= A.r)", LOCAL + PROJ[:1], "area: right-coordinate error == r refused")
M(107, F, "if (ur > 0 && fabsf(__fsub_rn(A.ur, ur)) > A.r)", "if (fabsf(__fsub_rn(A.ur, ur)) > A.r)", LOCAL + PROJ[:1], "area: the ur > 0 clause removed (monocular keypoints gated)")
M(108, F, "if (gate_right && A.gate == 1) {", "if (gate_right) {", FUSE + LOCAL[:2], "area: Fuse's queries take the right-coordinate radius test")
# chi2_accept
M(110, F, "(double)__fmul_rn(e2, inv) > 7.8);", "(double)__fmul_rn(e2, inv) > 5.99);", FUSE, "chi2: the stereo keypoints judged by the monocular bound")
M(111, F, "(double)__fmul_rn(e2, inv) > 5.99);", "(double)__fmul_rn(e2, inv) > 7.8);", FUSE, "chi2: the monocular keypoints judged by the stereo bound")
M(112, F, "(double)__fmul_rn(e2, inv) > 7.8);", "(double)__fmul_rn(e2, inv) >= 7.8);", FUSE, "chi2: stereo bound inclusive",
  "equivalent: the left side is a float widened to double and 7.8 is no float (nor is 5.99), so the two never compare equal")
M(113, F, "(double)__fmul_rn(e2, inv) > 5.99);", "(double)__fmul_rn(e2, inv) >= 5.99);", FUSE, "chi2: monocular bound inclusive",
  "equivalent: the left side is a float widened to double and 5.99 is no float, so the two never compare equal")
M(114, F, "    if (ur >= 0) {\n        const float er", "    if (ur > 0) {\n        const float er", FUSE, "chi2: a right coordinate of exactly 0 counts as monocular")
# frustum_body (+ rig form)
M(120, F, "if (z < 0.0f) ok = false;", "if (z <= 0.0f) ok = false;", LOCAL, "frustum: depth exactly 0 refused",
  note="no defined expectation: a point with z == 0 and x or y != 0 projects to +-inf and fails the image test either way; only the camera centre itself (x = y = z = 0, u = v = NaN) passes, and there the reference goes on to MapPoint::PredictScale with a distance of 0 - `(int)ceil(log(inf) / ..)`, an undefined conversion that gcc and the device answer differently")
M(121, F, "if (uu < F.min_x || uu > F.max_x) ok = false;", "if (uu <= F.min_x || uu > F.max_x) ok = false;", LOCAL, "frustum: u == mnMinX outside")
M(122, F, "if (uu < F.min_x || uu > F.max_x) ok = false;", "if (uu < F.min_x || uu >= F.max_x) ok = false;", LOCAL, "frustum: u == mnMaxX outside")
M(123, F, "(vv < F.min_y || vv > F.max_y)) ok = false;", "(vv <= F.min_y || vv > F.max_y)) ok = false;", LOCAL, "frustum: v == mnMinY outside")
M(124, F, "(vv < F.min_y || vv > F.max_y)) ok = false;", "(vv < F.min_y || vv >= F.max_y)) ok = false;", LOCAL, "frustum: v == mnMaxY outside")
M(125, F, "if (dist < minDistance || dist > maxDistance) ok = false;", "if (dist <= minDistance || dist > maxDistance) ok = false;", LOCAL, "frustum: distance == 0.8 min refused")
M(126, F, "if (dist < minDistance || dist > maxDistance) ok = false;", "if (dist < minDistance || dist >= maxDistance) ok = false;", LOCAL, "frustum: distance == 1.2 max refused")
M(127, F, "if (vcos < F.cos_limit) ok = false;", "if (vcos <= F.cos_limit) ok = false;", LOCAL, "frustum: viewing cosine == limit refused")
M(128, F, "!(F.far_points && depth > F.th_far)", "!(F.far_points && depth >= F.th_far)", LOCAL, "local points: depth == thFarPoints is far")
M(129, F, "float r = (double)vcos > 0.998 ? 2.5f : 4.0f;", "float r = (double)vcos >= 0.998 ? 2.5f : 4.0f;", LOCAL, "RadiusByViewingCos inclusive",
  "equivalent: vcos is a float widened to double and 0.998 is no float, so the two never compare equal")
M(130, F, "float r = (double)vcos > 0.998 ? 2.5f : 4.0f;", "float r = (double)vcos > 0.99 ? 2.5f : 4.0f;", LOCAL, "RadiusByViewingCos: 0.99 for 0.998")
M(131, F, "float r = (double)vcos > 0.998 ? 2.5f : 4.0f;", "float r = vcos > 0.998f ? 2.5f : 4.0f;", LOCAL, "RadiusByViewingCos compared in float")
M(132, F, "q.min_level = lvl - 1; q.max_level = lvl; q.active = 1; q.gate = 1;", "q.min_level = lvl; q.max_level = lvl; q.active = 1; q.gate = 1;", LOCAL, "local points: the level below the predicted one refused")
M(133, F, "if (F.th != 1.0f) r = __fmul_rn(r, F.th);", "r = __fmul_rn(r, F.th);", LOCAL, "local points: the radius always multiplied by th",
  "equivalent: r * 1.0f == r for every float r")
M(134, F, "const float r = (double)track2[4 * Ms + i] > 0.998 ? 2.5f : 4.0f;", "const float r = (double)track2[4 * Ms + i] > 0.99 ? 2.5f : 4.0f;", RIG, "rig camera 2: 0.99 for 0.998")
M(135, F, "track1[3 * Ms + i] > F1.th_far)", "track1[3 * Ms + i] >= F1.th_far)", RIG, "rig: depth == thFarPoints is far")
M(136, F, "const bool alive = (inl || inr) &&", "const bool alive = inl &&", RIG, "rig: a point seen by camera 2 alone is dropped")
M(137, F, "q.min_level = lvl - 1; q.max_level = lvl; q.active = 1;\n", "q.min_level = lvl; q.max_level = lvl; q.active = 1;\n", RIG, "rig camera 2: the level below the predicted one refused")
# project_point
M(140, F, "if (P.depth_test == 1 && z < 0.0f) ok = false;", "if (P.depth_test == 1 && z <= 0.0f) ok = false;", FUSE + SIM3, "projection: depth exactly 0 refused (z test)",
  note="no defined expectation: a point with z == 0 and x or y != 0 projects to +-inf and fails the image test either way; only the camera centre itself (x = y = z = 0, u = v = NaN) passes, and there the reference goes on to MapPoint::PredictScale with a distance of 0 - `(int)ceil(log(inf) / ..)`, an undefined conversion that gcc and the device answer differently")
M(141, F, "if (P.depth_test == 2 && invz < 0.0f) ok = false;", "if (P.depth_test == 2 && invz <= 0.0f) ok = false;", FUSE + SIM3 + PROJ[:2], "projection: 1 / z == 0 refused")
M(142, F, "if (u < P.min_x || u > P.max_x || v < P.min_y || v > P.max_y) ok = false; }", "if (u <= P.min_x || u >= P.max_x || v <= P.min_y || v >= P.max_y) ok = false; }", FUSE + SIM3 + PROJ[:2], "projection (Frame bounds): the border is outside")
M(143, F, "!(u >= P.min_x && u < P.max_x && v >= P.min_y && v < P.max_y)", "!(u > P.min_x && u < P.max_x && v > P.min_y && v < P.max_y)", FUSE + SIM3, "projection (IsInImage): the lower border is outside")
M(144, F, "!(u >= P.min_x && u < P.max_x && v >= P.min_y && v < P.max_y)", "!(u >= P.min_x && u <= P.max_x && v >= P.min_y && v <= P.max_y)", FUSE + SIM3, "projection (IsInImage): the upper border is inside")
M(145, F, "if (P.distance_test && (dist < min_inv || dist > max_inv)) ok = false;", "if (P.distance_test && (dist <= min_inv || dist > max_inv)) ok = false;", FUSE + SIM3, "projection: distance == lower limit refused")
M(146, F, "if (P.distance_test && (dist < min_inv || dist > max_inv)) ok = false;", "if (P.distance_test && (dist < min_inv || dist >= max_inv)) ok = false;", FUSE + SIM3, "projection: distance == upper limit refused")
M(147, F, "if (dot < __fmul_rn(0.5f, dist)) ok = false;", "if (dot <= __fmul_rn(0.5f, dist)) ok = false;", FUSE + SIM3, "projection: viewing angle of exactly 60 degrees refused")
M(148, F, "if (dot < __fmul_rn(0.5f, dist)) ok = false;", "if (dot < __fmul_rn(0.6f, dist)) ok = false;", FUSE + SIM3, "projection: viewing-angle bound 0.6 for 0.5")
# projection_queries_body
M(150, F, "(!(invz < 0.0f) && oct >= 0 && oct < F.nlevels)", "(!(invz <= 0.0f) && oct >= 0 && oct < F.nlevels)", PROJ, "last frame: 1 / z == 0 refused")
M(151, F, "if (!(u < F.min_x || u > F.max_x || v < F.min_y || v > F.max_y)) {", "if (!(u <= F.min_x || u >= F.max_x || v <= F.min_y || v >= F.max_y)) {", PROJ, "last frame / key frame: the image border is outside")
M(152, F, "if (!(dist3D < minDistance || dist3D > maxDistance)) {", "if (!(dist3D <= minDistance || dist3D > maxDistance)) {", PROJ, "key frame: distance == 0.8 min refused")
M(153, F, "if (!(dist3D < minDistance || dist3D > maxDistance)) {", "if (!(dist3D < minDistance || dist3D >= maxDistance)) {", PROJ, "key frame: distance == 1.2 max refused")
M(154, F, "q.min_level = n - 1; q.max_level = n + 1; q.active = 1; q.gate = 0;", "q.min_level = n - 1; q.max_level = n; q.active = 1; q.gate = 0;", PROJ, "key frame: the level above the predicted one refused")
M(155, F, "if (F.forward) { q.min_level = oct; q.max_level = -1; }", "if (F.forward) { q.min_level = oct + 1; q.max_level = -1; }", PROJ, "last frame, forward: the keypoint's own octave refused")
M(156, F, "else if (F.backward) { q.min_level = 0; q.max_level = oct; }", "else if (F.backward) { q.min_level = 0; q.max_level = oct - 1; }", PROJ, "last frame, backward: the keypoint's own octave refused")
M(157, F, "else { q.min_level = oct - 1; q.max_level = oct + 1; }", "else { q.min_level = oct; q.max_level = oct + 1; }", PROJ, "last frame: the octave below refused")
# fuse_query, fuse_best_free, k_fuse_candidates, sim3_choice
M(160, F, "A.min_level = n - 1; A.max_level = n; A.active = 1; A.gate = chi2_gate ? 2 : 0;", "A.min_level = n; A.max_level = n; A.active = 1; A.gate = chi2_gate ? 2 : 0;", FUSE + SIM3, "Fuse / Sim3: the level below the predicted one refused")
M(161, F, "A.min_level = n - 1; A.max_level = n; A.active = 1; A.gate = chi2_gate ? 2 : 0;", "A.min_level = n - 1; A.max_level = n + 1; A.active = 1; A.gate = chi2_gate ? 2 : 0;", FUSE + SIM3, "Fuse / Sim3: the level above the predicted one admitted")
M(162, F, "if (dist < best_dist) { best_dist = dist; best_idx = idx; }", "if (dist <= best_dist) { best_dist = dist; best_idx = idx; }", FUSE + SIM3, "Fuse / Sim3: the last of equal distances wins")
M(163, F, "if (bd > th_low) bi = -1;", "if (bd >= th_low) bi = -1;", FUSE, "Fuse: bestDist == TH_LOW refused")
M(164, F, "return (bi >= 0 && (float)bd <= max_dist) ? bi : -1;", "return (bi >= 0 && (float)bd < max_dist) ? bi : -1;", SIM3, "Sim3: bestDist == TH_LOW * ratioHamming refused")
M(165, F, "if (A.gate == 2 && !chi2_accept(A, k, R.ur[idx], g)) continue;", "", FUSE, "Fuse: the chi-square gate removed")
# accept bodies: local, last frame, rig
M(170, F, "accept = t.bestDist <= th_high && (LASTFRAME ||", "accept = t.bestDist < th_high && (LASTFRAME ||", LOCAL + PROJ[:2], "accept: bestDist == TH_HIGH refused")
M(171, F, "!(t.bestLevel == t.bestLevel2 && (float)t.bestDist > __fmul_rn(nnratio, (float)t.bestDist2)));", "!(t.bestLevel == t.bestLevel2 && (float)t.bestDist >= __fmul_rn(nnratio, (float)t.bestDist2)));", LOCAL, "accept: bestDist == mfNNratio * bestDist2 refused")
M(172, F, "!(t.bestLevel == t.bestLevel2 && (float)t.bestDist > __fmul_rn(nnratio, (float)t.bestDist2)));", "!((float)t.bestDist > __fmul_rn(nnratio, (float)t.bestDist2)));", LOCAL, "accept: the ratio test without the level-equality clause")
M(173, F, "const bool claims = accept && obs;", "const bool claims = accept;", LOCAL, "accept: a point without observations occupies its keypoint",
  "equivalent in the output: `claims` only makes later lanes of the round wait (dirty); what they then decide is read from s_occ, which takes the point's has_obs two lines below")
M(174, F, "if (obs) atomicOr(&s_occ[idx1 >> 5], 1u << (idx1 & 31));", "atomicOr(&s_occ[idx1 >> 5], 1u << (idx1 & 31));", LOCAL, "accept: a point without observations occupies its keypoint")
M(175, F, "if (best1.any() && t1.bestDist <= th_high) {", "if (best1.any() && t1.bestDist < th_high) {", RIG, "rig accept, camera 1: bestDist == TH_HIGH refused")
M(176, F, "if (best2.any() && t2.bestDist <= th_high) {", "if (best2.any() && t2.bestDist < th_high) {", RIG, "rig accept, camera 2: bestDist == TH_HIGH refused")
M(177, F, "if (!LASTFRAME && t1.bestLevel == t1.bestLevel2 && (float)t1.bestDist > __fmul_rn(nnratio, (float)t1.bestDist2)) end = true;",
  "if (!LASTFRAME && t1.bestLevel == t1.bestLevel2 && (float)t1.bestDist >= __fmul_rn(nnratio, (float)t1.bestDist2)) end = true;", RIG, "rig accept, camera 1: ratio test inclusive")
M(178, F, "if (LASTFRAME || !(t2.bestLevel == t2.bestLevel2 && (float)t2.bestDist > __fmul_rn(nnratio, (float)t2.bestDist2))) {",
  "if (LASTFRAME || !(t2.bestLevel == t2.bestLevel2 && (float)t2.bestDist >= __fmul_rn(nnratio, (float)t2.bestDist2))) {", RIG, "rig accept, camera 2: ratio test inclusive")
M(179, F, "if (!LASTFRAME && t1.bestLevel == t1.bestLevel2 && (float)t1.bestDist >", "if (!LASTFRAME && (float)t1.bestDist >", RIG, "rig accept, camera 1: the ratio test without the level-equality clause")
M(180, F, "if (!end && c2 > 0) {", "if (c2 > 0) {", RIG, "rig accept: camera 2 searched after a ratio-test rejection of camera 1")
# the rotation histogram
M(185, F, "if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);", "if (rot <= 0.0f) rot = __fadd_rn(rot, 360.0f);", PROJ + BOW[:3] + ["test_keyframe_search_gates.py"], "rotation: a difference of exactly 0 becomes 360 (bin 12 instead of bin 0)")
M(186, F, "return bin == 30 ? 0 : bin;", "return bin == 29 ? 0 : bin;", PROJ + BOW[:3], "rotation: bin 29 folded onto bin 0",
  note="equivalent: rot lies in [0, 360) and the factor is 1 / 30, so bin = round(rot / 30) is at most 12 (the reference's HISTO_LENGTH quirk); neither 29 nor 30 ever occurs")
M(187, F, "if ((float)max2 < __fmul_rn(0.1f, (float)max1)) { ind2 = -1; ind3 = -1; }", "if ((float)max2 <= __fmul_rn(0.1f, (float)max1)) { ind2 = -1; ind3 = -1; }", PROJ + BOW[:3], "three maxima: a second bin of exactly 10 % dropped")
M(188, F, "else if ((float)max3 < __fmul_rn(0.1f, (float)max1)) ind3 = -1;", "else if ((float)max3 <= __fmul_rn(0.1f, (float)max1)) ind3 = -1;", PROJ + BOW[:3], "three maxima: a third bin of exactly 10 % dropped")
M(189, F, "if (sz > max1) { max3 = max2;", "if (sz >= max1) { max3 = max2;", PROJ + BOW[:3], "three maxima: the last of equal bins is the first maximum")
# bow_search_core (SearchForTriangulation), k_sft_*
M(190, F, "const bool stereo2 = ur2[idx2] >= 0;", "const bool stereo2 = ur2[idx2] > 0;", BOW, "triangulation search: a right coordinate of exactly 0 counts as monocular")
M(191, F, "if (P.only_stereo && !stereo2) continue;", "", BOW, "triangulation search: the only_stereo gate on KF2 removed")
M(192, F, "if (dist > P.th_low) continue;", "if (dist >= P.th_low) continue;", BOW, "triangulation search: distance == TH_LOW refused")
M(193, F, "< __fmul_rn(100.f, P.scale2[k2.octave])) continue;", "<= __fmul_rn(100.f, P.scale2[k2.octave])) continue;", BOW, "triangulation search: epipole distance == bound refused")
M(194, F, "if (!stereo1 && !stereo2 && !(KB8 && P.nleft1 >= 0)) {", "if (!stereo1 && !(KB8 && P.nleft1 >= 0)) {", BOW, "triangulation search: epipole test for stereo keypoints of KF2")
M(195, F, "if (!(z > 0.0001f)) continue;", "if (!(z > 0.0f)) continue;", BOW, "triangulation search (KB8): depth gate 0 for 1e-4")
M(196, F, "if (!((double)dsqr < 3.84 * (double)P.sigma2_2[k2.octave])) continue;", "if (!((double)dsqr <= 3.84 * (double)P.sigma2_2[k2.octave])) continue;", BOW, "triangulation search: epipolar distance == bound accepted")
M(197, F, "if (!((double)dsqr < 3.84 * (double)P.sigma2_2[k2.octave])) continue;", "if (!((double)dsqr < 5.99 * (double)P.sigma2_2[k2.octave])) continue;", BOW, "triangulation search: 5.99 for 3.84")
M(198, F, "((unsigned)dist << 16) | (unsigned)(0xFFFF - j);", "((unsigned)dist << 16) | (unsigned)j;", BOW, "triangulation search: the first of equal distances wins",
  more=[("feat2[0xFFFF - (int)(best & 0xFFFF)];", "feat2[(int)(best & 0xFFFF)];")])
M(199, F, "if (a >= 0 && !flags[idx1] && !(S.P.only_stereo && !stereo1)) {", "if (a >= 0 && !flags[idx1]) {", BOW, "triangulation search (resident): the only_stereo gate on KF1 removed")
M(200, F, "const bool stereo1 = k1.ur[idx1] >= 0;", "const bool stereo1 = k1.ur[idx1] > 0;", BOW, "triangulation search (resident): KF1 right coordinate of exactly 0 counts as monocular")
# bow_match_node, bow_prune_body
M(205, F, "const bool pass = th_inclusive ? bestDist1 <= th_low : bestDist1 < th_low;", "const bool pass = th_inclusive ? bestDist1 < th_low : bestDist1 <= th_low;", BOW, "SearchByBoW: the TH_LOW comparisons of the two forms swapped")
M(206, F, "if (pass && (float)bestDist1 < __fmul_rn(nnratio, (float)bestDist2)) {", "if (pass && (float)bestDist1 <= __fmul_rn(nnratio, (float)bestDist2)) {", BOW, "SearchByBoW: ratio test inclusive")
M(207, F, "if ((int)(mr >> 16) <= th_low) {", "if ((int)(mr >> 16) < th_low) {", BOW, "SearchByBoW (rig): camera 2's best == TH_LOW refused")
M(208, F, "if (RIG && pass) {", "if (RIG) {", BOW, "SearchByBoW (rig): camera 2 considered though camera 1's best failed TH_LOW")
M(209, F, "if (!mp1[idx1]) continue;", "", BOW, "SearchByBoW: features of K1 without a good map point searched")
M(210, F, "if (el2 && !el2[idx2]) continue;", "", BOW, "SearchByBoW: ineligible features of K2 are candidates")
M(211, F, "if (!top.keeps(bin_of(i, j))) { m[i] = -1; nm--; }", "if (top.keeps(bin_of(i, j))) { m[i] = -1; nm--; }", BOW, "rotation pruning negated")
# the resident map's state tests
M(220, F, "return slot >= 0 && state[slot] == kMapPresent ? slot : -1;", "return slot >= 0 && (state[slot] & kMapPresent) ? slot : -1;", MAP, "map_visit: a bad point is visited")
M(221, F, "ok = (st & kMapPresent) && !(rows && (st & kMapBad)) && !excluded[o];", "ok = (st & kMapPresent) && !(st & kMapBad) && !excluded[o];", MAP + PROJ[:2], "rows gather: the last-frame form refuses bad points too")
M(222, F, "ok = (st & kMapPresent) && !(rows && (st & kMapBad)) && !excluded[o];", "ok = (st & kMapPresent) && !excluded[o];", MAP + PROJ[:2], "rows gather: the key-frame form admits bad points")
M(223, F, "ok = (st & kMapPresent) && !(rows && (st & kMapBad)) && !excluded[o];", "ok = (st & kMapPresent) && !(rows && (st & kMapBad));", MAP + PROJ[:2], "rows gather: the caller's exclusion flag ignored")
M(224, F, "(R.rule == kRowHoldsPoint ? (state[slot] & kMapPresent) != 0 : state[slot] == kMapPresent)", "(R.rule == kRowHoldsPoint ? state[slot] == kMapPresent : state[slot] == kMapPresent)", MAP + BOW[:1], "row flags: kRowHoldsPoint refuses bad points")
M(225, F, "(R.rule == kRowHoldsPoint ? (state[slot] & kMapPresent) != 0 : state[slot] == kMapPresent)", "(R.rule == kRowHoldsPoint ? (state[slot] & kMapPresent) != 0 : (state[slot] & kMapPresent) != 0)", MAP + BOW[:1], "row flags: kRowHoldsGoodPoint admits bad points")
M(226, F, "out = st == kMapPresent ? slot : (st & kMapPresent) ? -2 : -1;", "out = (st & kMapPresent) ? slot : -1;", MAP + FUSE[:2], "fuse kf slots: a bad point in the key frame is fused with")
M(227, F, "out = st == kMapPresent ? slot : (st & kMapPresent) ? -2 : -1;", "out = st == kMapPresent ? slot : -1;", MAP + FUSE[:2], "fuse kf slots: a bad point in the key frame reads as an empty entry")
M(228, F, "const uint8_t bad = (uint8_t)(state[slot] != kMapPresent);", "const uint8_t bad = (uint8_t)((state[slot] & kMapPresent) == 0);", MAP + FUSE[:2] + SIM3[:2], "set table: a bad point is not skipped")
M(229, F, "if (q == 0 && (S.state[slot] & kMapPresent)) S.state[slot] = st;", "if (q == 0) S.state[slot] = st;", MAP, "set_bad: a slot that holds nothing becomes present")
M(230, F, "if (t > base && p < (unsigned)M) skip", "if (t >= base && p < (unsigned)M) skip", MAP + FUSE[:2] + SIM3[:2], "skip listed: a stamp of an earlier call counts as in the set",
  note="equivalent: top = base + M, so a stamp t == base gives the position p = top - t = M, and the clause p < M beside it refuses exactly that value")
# k_stereo_from_depth
M(235, F, "if (d > 0) {\n                const float xu", "if (d >= 0) {\n                const float xu", ["test_local_points_batch.py", "test_emu_search.py", "test_frame_reference.py"], "RGB-D: depth 0 is a measurement")
# the compacted pair list of a Fuse batch: k_fuse_pairs, k_fuse_pair_scan_tiles, k_fuse_pair_scan_sums, fuse_pair_kf_slot
# (`total > cap` is not mutated towards writing: the records of a list longer than cap would lie behind the array.  `at >= total` only keeps a store inside the list.)
PAIRS = ["test_fuse_pairs.py"]
M(240, F, "const bool keep = feat >= 0;", "const bool keep = feat > 0;", PAIRS, "fuse pairs: a pair with feature 0 is left out")
M(241, F, "int at = at0 + __popcll(bal & ((1ull << lane) - 1ull));", "int at = at0 + __popcll(bal & ((2ull << lane) - 1ull));", PAIRS, "fuse pairs: the rank inside a wave counts the lane itself")
M(242, F, "for (int w = 0; w < wave; w++) at += wave_cnt[w];\n    if (at >= total)", "for (int w = 0; w <= wave; w++) at += wave_cnt[w];\n    if (at >= total)", PAIRS,
  "fuse pairs: the rank inside a chunk counts the lane's own wave")
M(243, F, "if (!keep || total > cap) return;", "if (!keep || total >= cap) return;", PAIRS, "fuse pairs: a list of exactly cap entries is not written")
M(244, F, "if (i < n) chunk_off[i] = incl - v;", "if (i < n) chunk_off[i] = incl;", PAIRS, "fuse pair scan: chunk offsets inclusive")
M(245, F, "tile_off[j] = run - tile_sum[j]; }", "tile_off[j] = run; }", PAIRS, "fuse pair scan: tile offsets inclusive")
M(246, F, "if (slot < 0) return -1;\n    const uint8_t st = state[slot];\n    if (!(st & kMapPresent)) return -1;", "if (slot < 0) return -2;\n    const uint8_t st = state[slot];\n    if (!(st & kMapPresent)) return -1;",
  PAIRS, "fuse pair kf slot: an empty row entry reads as a bad point")
M(247, F, "if (!(st & kMapPresent)) return -1;\n    return (st & kMapBad)", "if (!(st & kMapPresent)) return -2;\n    return (st & kMapBad)", PAIRS, "fuse pair kf slot: a slot that holds nothing reads as a bad point")
M(248, F, "if (!(st & kMapPresent)) return -1;\n    return (st & kMapBad)", "if (!(st & kMapPresent)) return slot;\n    return (st & kMapBad)", PAIRS, "fuse pair kf slot: a slot that holds nothing is fused with")
M(249, F, "return (st & kMapBad) ? -2 : slot;", "return slot;", PAIRS, "fuse pair kf slot: a bad point in the key frame is fused with")
M(250, F, "return (st & kMapBad) ? -2 : slot;", "return (st & kMapBad) ? -1 : slot;", PAIRS, "fuse pair kf slot: a bad point in the key frame reads as an empty entry")
M(251, F, "if (blockIdx.x == 0) start[k] = at0;\n        if (chunk == 0) start[gridDim.y] = total;", "if (blockIdx.x == 0) start[k] = at0;\n        if (chunk == 0) start[gridDim.y] = total - 1;", PAIRS,
  "fuse pairs: start[K] one short of the list")

# ---- k_vocab.hip ---------------------------------------------------------------------------------------------------------------------------------------------
F = "k_vocab.hip"
VOC = ["test_emu_vocab.py", "test_emu_kfdb.py"]
M(300, F, "key = ((unsigned)dist << 8) | (unsigned)c;", "key = ((unsigned)dist << 8) | (unsigned)(255 - c);", VOC, "descend: the last child of equal distances wins",
  more=[("slot = cs + (int)(best & 0xFFu);", "slot = cs + 255 - (int)(best & 0xFFu);")])
M(301, F, "if (i < n && wt_[i] > 0) {", "if (i < n && wt_[i] >= 0) {", VOC, "assemble: stopped words (weight 0) enter the vectors")
M(302, F, "if (weighting <= 1) for (int t = s + 1;", "if (weighting < 1) for (int t = s + 1;", VOC, "assemble: TF counts a word once")
M(303, F, "if (weighting <= 1) for (int t = s + 1;", "if (weighting <= 2) for (int t = s + 1;", VOC, "assemble: IDF adds the weight per feature")
M(304, F, "if (weighting <= 1 && norm == 0 && nu > 0) {", "if (weighting < 1 && norm == 0 && nu > 0) {", VOC, "assemble: TF without normalisation not divided by the word count")
M(305, F, "if (weighting <= 1 && norm == 0 && nu > 0) {", "if (weighting <= 1 && nu > 0) {", VOC, "assemble: divided by the word count although normalised")
M(306, F, "if (norm == 1) for (int u = 0; u < nu; u++) acc = acc + fabs(", "if (norm == 2) for (int u = 0; u < nu; u++) acc = acc + fabs(", VOC, "assemble: L1 and L2 norms swapped")
M(307, F, "if (nv > 0.0) for", "if (nv >= 0.0) for", VOC, "assemble: a zero norm divides",
  "equivalent: every value is a sum of weights > 0 (stopped words are filtered above), so nv == 0 only when nu == 0, and then the loop is empty")
M(310, F, "if (qw[mid] < w) lo = mid + 1; else hi = mid;", "if (qw[mid] <= w) lo = mid + 1; else hi = mid;", VOC, "kfdb: the word search steps over an equal id")
M(311, F, "const int minc = (int)((float)mx * 0.8f);", "const int minc = (int)((float)mx * 0.7f);", VOC, "kfdb: minCommonWords 0.7 of the maximum")
M(312, F, "const int sc = (score_all || v > minc) ? 1 : 0;", "const int sc = (score_all || v >= minc) ? 1 : 0;", VOC, "kfdb: minCommonWords inclusive")
M(313, F, "if (j < lane) rank++; else if (j > lane) last = false;", "if (j > lane) rank++; else if (j < lane) last = false;", VOC, "kfdb: records of equal first position in reverse order")
M(314, F, "if (sv != 0.0) t = __dmul_rn(vi, wi) / sv; else hit = 0;", "if (sv == 0.0) t = __dmul_rn(vi, wi) / sv; else hit = 0;", VOC, "kfdb chi-square: the zero test negated")
M(315, F, "score = acc >= 1.0 ? 1.0 :", "score = acc > 1.0 ? 1.0 :", VOC, "kfdb L2: clamp exclusive",
  "equivalent: at acc == 1.0 the other arm gives 1.0 - sqrt(1.0 - 1.0) = 1.0 as well")
M(316, F, "if (scoring == 0) score = -acc / 2.0;", "if (scoring == 5) score = -acc / 2.0;", VOC, "kfdb: the L1 finisher on the dot product instead")
M(317, F, "else if (scoring == 1) score = acc >= 1.0", "else if (scoring == 5) score = acc >= 1.0", VOC, "kfdb: the L2 finisher on the dot product instead")
M(318, F, "else if (scoring == 2) score = __dmul_rn(2.0, acc);", "else if (scoring == 5) score = __dmul_rn(2.0, acc);", VOC, "kfdb: the chi-square finisher on the dot product instead")

# ---- k_describe.hip: k_layout and fast_atan2_deg ------------------------------------------------------------------------------------------------------------
# (bucket_of's imin / imax clamp an index into the row histogram: address arithmetic, not mutated)
F = "k_describe.hip"
LAYOUT = ["test_emu_parity.py", "test_emu_fuzz.py", "test_knn2_constructed.py"]
ATAN = ["test_model_sweep.py", "test_models.py", "test_orient_chain.py"]
M(400, F, "xf >= (float)lap0 && xf <= (float)lap1;", "xf > (float)lap0 && xf <= (float)lap1;", LAYOUT, "layout: x == lapping begin is monocular")
M(401, F, "xf >= (float)lap0 && xf <= (float)lap1;", "xf >= (float)lap0 && xf < (float)lap1;", LAYOUT, "layout: x == lapping end is monocular")
M(402, F, "if (x < 0) a = __fsub_rn(180.f, a);", "if (x <= 0) a = __fsub_rn(180.f, a);", ATAN, "fastAtan2: x == 0 mirrored (differs at x = y = 0 only: 180 for 0)")
M(403, F, "if (y < 0) a = __fsub_rn(360.f, a);", "if (y <= 0) a = __fsub_rn(360.f, a);", ATAN, "fastAtan2: y == 0 gives 360 - a")
M(404, F, "if (ax >= ay) {", "if (ax > ay) {", ATAN, "fastAtan2: |x| == |y| takes the 90 - a branch")


# ==== the extraction half: k_describe (rest), k_fast, k_quadtree, k_image, blur_body.h, k_input and the host tables of orbx_api.cpp ================================
# These kernels write into arrays sized from the decisions themselves, so the safety rule is stricter: no mutant may let a kernel emit more items into a
# fixed-capacity array than the array was sized for (profiles/emu_mutants_extract/README.md, "What is not in the list", names every line left out for that).
# The whole of tests/test_emu_parity.py takes minutes on the emulator (its 4127-pixel cases): the groups name the small cases by node id, the new constructed
# tests first.
NEW = "test_extract_decisions.py"
SMALL = ["test_emu_parity.py::test_extractor_stagewise_and_final[%s]" % c for c in
         ("small_376x240_n500", "small_lap_partial", "small_noise", "small_threshold_fallback", "small_280x260_wide_cells", "min_239x239_noise_n1000")]
EXTRACT = [NEW] + SMALL + ["test_emu_parity.py::test_extreme_fast_thresholds", "test_emu_parity.py::test_other_parameters_and_gauss_variant", "test_emu_fuzz.py"]
IMAGE = EXTRACT + ["test_emu_parity.py::test_pyramid_one_launch_emulated", "test_emu_parity.py::test_row_ends_of_every_width", "test_emu_pyramid_export.py"]
DESCRIBE = EXTRACT + ["test_orient_chain.py"]
DESCRIBE_STEREO = DESCRIBE + ["test_emu_parity.py::test_batch_and_stereo_and_knn", "test_stereo_chain.py"]
INPUT = ["test_emu_input.py"]
LOOSER = ("equivalent in the output: the quick test of phase A only chooses which pixels phase B scores; phase B (fast_score_pk) decides exactly and writes a score "
          "only where it is positive, so a looser quick test lists more pixels and changes no score; a list that fills sooner gives the corner list up, and the "
          "list-free NMS (C', D') computes the same set from the same score tile")

# ---- k_describe.hip: k_orient_brief and the rest of k_layout -------------------------------------------------------------------------------------------------------
F = "k_describe.hip"
M(405, F, "au <= kHalfPatch && au <= um[trip];", "au <= kHalfPatch && au < um[trip];", DESCRIBE, "IC_Angle: the disc's rim columns (|u| == umax[|v|]) left out")
M(406, F, "const bool on = av <= kHalfPatch &&", "const bool on = av < kHalfPatch &&", DESCRIBE, "IC_Angle: rows v = +-15 left out")
M(407, F, "(uint32_t)(u + 16) << (8 * j)", "(uint32_t)(u + 17) << (8 * j)", DESCRIBE, "IC_Angle: column weight biased by 17 against the correction by 16")
M(408, F, "int m10 = (int)du - 16 * ds;", "int m10 = (int)du - 15 * ds;", DESCRIBE, "IC_Angle: bias correction 15 * sum")
M(409, F, "m01 += mul24(-kHalfPatch + 8 * trip + r8, s);", "m01 += mul24(kHalfPatch - 8 * trip - r8, s);", DESCRIBE, "IC_Angle: sign of m01's row weight")
M(410, F, "ORBX_BALLOT(t0v[r] < t1v[r]);", "ORBX_BALLOT(t0v[r] <= t1v[r]);", DESCRIBE, "BRIEF: equal samples set the bit")
M(411, F, "__fadd_rn(__fmul_rn(px0[r], bb), __fmul_rn(py0[r], a))", "__fsub_rn(__fmul_rn(px0[r], bb), __fmul_rn(py0[r], a))", DESCRIBE, "BRIEF: sign in the first point's row")
M(412, F, "__fsub_rn(__fmul_rn(px0[r], a), __fmul_rn(py0[r], bb))", "__fadd_rn(__fmul_rn(px0[r], a), __fmul_rn(py0[r], bb))", DESCRIBE, "BRIEF: sign in the first point's column")
M(413, F, "__fadd_rn(__fmul_rn(px1[r], bb), __fmul_rn(py1[r], a))", "__fsub_rn(__fmul_rn(px1[r], bb), __fmul_rn(py1[r], a))", DESCRIBE, "BRIEF: sign in the second point's row")
M(414, F, "__fsub_rn(__fmul_rn(px1[r], a), __fmul_rn(py1[r], bb))", "__fadd_rn(__fmul_rn(px1[r], a), __fmul_rn(py1[r], bb))", DESCRIBE, "BRIEF: sign in the second point's column")
M(415, F, "if (lvl[k] != 0) xf = __fmul_rn(xf, s_scale[lvl[k]]);", "if (lvl[k] > 1) xf = __fmul_rn(xf, s_scale[lvl[k]]);", DESCRIBE, "layout: level 1's x not scaled for the lapping test")
M(416, F, "if (my_level != 0) { xf = __fmul_rn(xf, my_scale);", "if (my_level > 1) { xf = __fmul_rn(xf, my_scale);", DESCRIBE, "records: level 1 not scaled")
M(417, F, "if (l != 0) yf = __fmul_rn(yf, s_scale[l]);", "if (l > 1) yf = __fmul_rn(yf, s_scale[l]);", DESCRIBE_STEREO, "row index: level 1's band from the unscaled y")
M(418, F, "aux.x = (int)floorf(__fsub_rn(yf, r));", "aux.x = (int)ceilf(__fsub_rn(yf, r));", DESCRIBE_STEREO, "stereo band: first row rounded up")
M(419, F, "aux.y = (int)ceilf(__fadd_rn(yf, r));", "aux.y = (int)floorf(__fadd_rn(yf, r));", DESCRIBE_STEREO, "stereo band: last row rounded down")
M(420, F, "fin[k] = lapf[k] ? total - 1 - pl : pm;", "fin[k] = lapf[k] ? pm : total - 1 - pl;", DESCRIBE, "layout: lapping keypoints from the front, monocular ones from the back")
M(421, F, "if (lvl[k] != 0) xf = __fmul_rn(xf, s_scale[lvl[k]]);", "xf = __fmul_rn(xf, s_scale[lvl[k]]);", DESCRIBE, "layout: level 0 scaled as well",
  "equivalent: the scale of level 0 is 1.0f (init_tables, csrc/orbx_api.cpp: h->scale[0] = 1.0f) and x * 1.0f == x for every float")
# (the band's half-height 2 * scale is written twice: the record's band and the row index's first row.  Only narrower bands are mutated: the matcher's look-back
# over the row buckets is sized for 2 * scale by the host - orbm_stereo_match, `lookback` - and a wider band is not covered by that size argument)
M(422, F, "const float r = __fmul_rn(2.0f, my_scale);", "const float r = __fmul_rn(1.0f, my_scale);", DESCRIBE_STEREO, "stereo band: half-height 1 * scale in the records")
M(423, F, "__fsub_rn(yf, __fmul_rn(2.0f, s_scale[l]))", "__fsub_rn(yf, __fmul_rn(1.0f, s_scale[l]))", DESCRIBE_STEREO, "row index: first row from a half-height of 1 * scale")

# ---- k_fast.hip ----------------------------------------------------------------------------------------------------------------------------------------------------
F = "k_fast.hip"
CAP = ("-DORBX_FAST_LIST_CAP=200",)
M(500, F, "sA = mA > t0 ? mA - 1 : 0;", "sA = mA >= t0 ? mA - 1 : 0;", EXTRACT, "FAST score: arc difference == t is a corner (entry A)")
M(501, F, "sB = mB > t0 ? mB - 1 : 0;", "sB = mB >= t0 ? mB - 1 : 0;", EXTRACT, "FAST score: arc difference == t is a corner (entry B)")
M(502, F, "sA = mA > t0 ? mA - 1 : 0;", "sA = mA > t0 + 1 ? mA - 1 : 0;", EXTRACT, "FAST score: arc difference == t + 1 is no corner (entry A)")
M(503, F, "sB = mB > t0 ? mB - 1 : 0;", "sB = mB > t0 + 1 ? mB - 1 : 0;", EXTRACT, "FAST score: arc difference == t + 1 is no corner (entry B)")
M(504, F, "sA = mA > t0 ? mA - 1 : 0;", "sA = mA > t0 ? mA : 0;", EXTRACT, "FAST score: the arc difference itself (entry A)")
M(505, F, "sB = mB > t0 ? mB - 1 : 0;", "sB = mB > t0 ? mB : 0;", EXTRACT, "FAST score: the arc difference itself (entry B)")
M(506, F, "const int td = (t0 + 1) >> 1;", "const int td = (t0 + 2) >> 1;", EXTRACT, "quick test: td one higher for even thresholds (stricter)")
M(507, F, "Cd = (uint32_t)(td - 1) * 0x01010101u,", "Cd = (uint32_t)td * 0x01010101u,", EXTRACT, "quick test: dark bound V - td instead of V - td + 1 (stricter)")
M(508, F, "Tb = (uint32_t)td * 0x01010101u;", "Tb = (uint32_t)(td + 1) * 0x01010101u;", EXTRACT, "quick test: bright bound V + td + 1 (stricter)")
M(509, F, "Tb = (uint32_t)td * 0x01010101u;", "Tb = (uint32_t)(td - 1) * 0x01010101u;", EXTRACT, "quick test: bright bound V + td - 1 (looser)", LOOSER + " (t0 >= 1 in this branch, so td - 1 >= 0)")
M(510, F, "const uint32_t Qd = x & (mx - (mx >> 7));", "const uint32_t Qd = x & kL7;", EXTRACT, "quick test: max(V - td + 1, 0) without the saturation at 0",
  "equivalent in the output: where V - td + 1 < 0 the byte of x is 128 + V - td + 1 in 1..127, so the mutant compares the ring with a bound above 0 where the kernel "
  "compares with 0 (every ring pixel `not dark`, SD = 0); a pixel with v - t0 < 0 has no dark corner, and what the mutant lists in addition phase B scores 0.  " + LOOSER)
M(511, F, "const uint32_t Pb = y ^ (y & (my - (my >> 7)));", "const uint32_t Pb = y;", EXTRACT, "quick test: min(V + td, 128) without the saturation at 128")
M(512, F, "if (t0 >= 1) {", "if (t0 >= 2) {", EXTRACT, "quick test: threshold 1 takes the score-everything branch", LOOSER)
M(513, F, "if (t0 >= 1) {", "if (t0 >= 0) {", EXTRACT, "quick test: threshold 0 goes through the byte arithmetic (td = 0)")
for _i, (_a, _b) in enumerate((("q0", "q4"), ("q1", "q5"), ("q2", "q6"), ("q3", "q7"))):
    M(514 + _i, F, "((%s - Qd) & (%s - Qd))" % (_a, _b), "((%s - Qd) | (%s - Qd))" % (_a, _b), EXTRACT, "quick test, dark: pair (%s, %s) needs BOTH ring pixels dark (stricter)" % (_a, _b))
    M(518 + _i, F, "((%s - Pb) | (%s - Pb))" % (_a, _b), "((%s - Pb) & (%s - Pb))" % (_a, _b), EXTRACT, "quick test, bright: pair (%s, %s) needs BOTH ring pixels bright (stricter)" % (_a, _b))
M(522, F, " | ((q3 - Qd) & (q7 - Qd));", ";", EXTRACT, "quick test, dark: the pair (6, 14) dropped (looser)", LOOSER)
M(523, F, " & ((q3 - Pb) | (q7 - Pb));", ";", EXTRACT, "quick test, bright: the pair (6, 14) dropped (looser)", LOOSER)
M(524, F, "const uint32_t ANY = SD | SB, BOTH = SD & SB;", "const uint32_t ANY = SD | SB, BOTH = 0u;", EXTRACT, "dual polarity: no second (dark) entry for a pixel listed for both")
M(525, F, "((SB & (0x80u << (8 * j))) ? kEntBright : 0)", "((SD & (0x80u << (8 * j))) ? 0 : kEntBright)", EXTRACT, "dual polarity: the first entry of a pixel listed for both is dark too")
M(526, F, "if (ORBX_IN_BALLOT(bald[j])) *lp++ = (uint16_t)(toff + j);", "if (ORBX_IN_BALLOT(bald[j])) *lp++ = (uint16_t)((toff + j) | kEntBright);", EXTRACT, "dual polarity: the second entry is bright too")
M(527, F, "if (sA > 0) sc[oA] = (uint8_t)sA;", "if (sA >= 0) sc[oA] = (uint8_t)sA;", EXTRACT, "score tile: a zero score overwrites the other polarity's (entry A)")
M(528, F, "if (hasB && sB > 0) sc[oB] = (uint8_t)sB;", "if (hasB && sB >= 0) sc[oB] = (uint8_t)sB;", EXTRACT, "score tile: a zero score overwrites the other polarity's (entry B)")
M(529, F, "if (hasB && sB > 0) sc[oB] = (uint8_t)sB;", "if (sB > 0) sc[oB] = (uint8_t)sB;", EXTRACT, "score tile: the hasB clause removed",
  "equivalent: without a second entry eB = eA (the line above), so sB == sA and oB == oA: the same byte is written twice")
# NMS strictness, one neighbour at a time: `c[n] - 1` makes the comparison with that neighbour >= and leaves the seven others strict.  Of two adjacent pixels one
# still sees the other through a strict comparison, so no two adjacent pixels survive and the count stays within ((iw + 1) / 2) * ((ih + 1) / 2), the cell's slots;
# a score-0 pixel of the list-free path still has seven neighbours >= 0 and does not survive.
_NB = (("c[-wp - 1]", "upper left"), ("c[-wp]", "upper"), ("c[-wp + 1]", "upper right"), ("c[-1]", "left"), ("c[1]", "right"), ("c[wp - 1]", "lower left"), ("c[wp]", "lower"),
       ("c[wp + 1]", "lower right"))
_M0 = "const int m0 = imax(imax((int)c[-wp - 1], (int)c[-wp]), imax((int)c[-wp + 1], (int)c[-1]));"
_M1 = "const int m1 = imax(imax((int)c[1], (int)c[wp - 1]), imax((int)c[wp], (int)c[wp + 1]));"
for _i, (_n, _w) in enumerate(_NB):
    _line = _M0 if _i < 4 else _M1
    _mut = _line.replace("(int)%s" % _n, "(int)%s - 1" % _n)
    if _i < 4:
        M(530 + _i, F, "zero frame\n                " + _line, "zero frame\n                " + _mut, EXTRACT, "NMS (corner list): a tie with the %s neighbour survives" % _w)
        M(540 + _i, F, "const int s = c[0];\n            " + _line, "const int s = c[0];\n            " + _mut, EXTRACT, "NMS (list-free): a tie with the %s neighbour survives" % _w, defines=CAP)
    else:
        M(530 + _i, F, _line + "\n                keep = s > imax(m0, m1);", _mut + "\n                keep = s > imax(m0, m1);", EXTRACT, "NMS (corner list): a tie with the %s neighbour survives" % _w)
        M(540 + _i, F, _line + "\n            kf[o]", _mut + "\n            kf[o]", EXTRACT, "NMS (list-free): a tie with the %s neighbour survives" % _w, defines=CAP)
M(550, F, "const int t0 = pass == 0 ? iniTh : minTh;", "const int t0 = pass == 0 ? iniTh : iniTh;", EXTRACT, "second run: at iniTh again")
M(551, F, "const int t0 = pass == 0 ? iniTh : minTh;", "const int t0 = pass == 0 ? iniTh : minTh + 1;", EXTRACT, "second run: at minTh + 1")
M(552, F, "if (base > 0 || pass == 1 || minTh >= iniTh) break;", "if (base > 0 || pass == 1 || minTh > iniTh) break;", EXTRACT, "second run: also when minTh == iniTh",
  "equivalent: the second run only happens for base == 0, and at the same threshold it computes the same empty set again")
M(553, F, "if (base > 0 || pass == 1 || minTh >= iniTh) break;", "if (base > 0 || pass == 1) break;", EXTRACT, "second run: the minTh >= iniTh clause removed (a higher minTh is run)",
  "equivalent: a strict 3x3 maximum with score >= minTh > iniTh is one with score >= iniTh too, so a cell that is empty at iniTh is empty at every higher threshold")
M(554, F, "if (wpr <= kFastPitch) fast_cell<kFastPitch>", "if (wpr < kFastPitch) fast_cell<kFastPitch>", EXTRACT, "window of exactly kFastPitch bytes takes the variable-pitch form",
  "equivalent: at wpr == kFastPitch the variable pitch wp = wpr is kFastPitch too; both forms lay the same tile out and the host sizes it with that pitch (configure, csrc/orbx_api.cpp: wp = gx1 - gx0 <= kFastPitch ? ..)")
M(555, F, "if (cnt + trip > list_cap) {                         // wave-uniform", "if (cnt + trip >= list_cap) {                         // wave-uniform", EXTRACT,
  "list flush: one trip earlier", "equivalent in the output: when the pending survivors are scored does not change their scores", defines=CAP)
M(556, F, "if (cnt + trip > list_cap) { corners_listed = false;", "if (cnt + trip >= list_cap) { corners_listed = false;", EXTRACT, "list overflow: given up when the trip fits exactly",
  "equivalent in the output: the list-free NMS and compaction (C', D') compute the same set in the same row-major order from the same score tile", defines=CAP)
# the ordered lists: phase A appends in (row, dword, byte) order, phase B compacts in place and in order, phase C writes the survivors in list order
# (tests/test_fast_ordered_lists.py; profiles/fast_ordered_lists/README.md).  Every mutant keeps its writes inside the entries the trip owns (ranks only shrink).
ORDER = ["test_fast_ordered_lists.py::test_ordered_lists_emulated", "test_fast_ordered_lists.py::test_mid_cell_flush_keeps_the_order"]
_RANK = "int r = nc + lanes_below(balB, lanes_below(balA));"
M(560, F, _RANK, "int r = nc + lanes_below(balB);", ORDER, "corner list: the rank without the even corners of the lanes below")
M(561, F, _RANK, "int r = nc + lanes_below(balA);", ORDER, "corner list: the rank without the odd corners of the lanes below")
M(562, F, "if (ORBX_IN_BALLOT(balA)) list[r++] = (uint16_t)oA;", "if (ORBX_IN_BALLOT(balA)) list[r] = (uint16_t)oA;", ORDER, "corner list: the odd entry's rank without its own lane's even entry")
_DUAL = "                    if (ORBX_IN_BALLOT(bal[j])) *lp++ = first_entry(j);\n                    if (ORBX_IN_BALLOT(bald[j])) *lp++ = (uint16_t)(toff + j);\n                }"
M(563, F, _DUAL, "                    if (ORBX_IN_BALLOT(bal[j])) *lp++ = first_entry(j);\n                }\n                for (int j = 0; j < 4; j++) {\n"
  "                    if (ORBX_IN_BALLOT(bald[j])) *lp++ = (uint16_t)(toff + j);\n                }", ORDER, "survivor list: a lane's second (dark) entries behind all of its first entries")
M(564, F, "            base += __popcll(bal);\n        }\n    } else {", "            base = __popcll(bal);\n        }\n    } else {", ORDER, "phase C: `base` does not carry from one trip of 64 corners to the next")
M(565, F, "mul24(y1, 4096 - wp)", "mul24(y1, 4095 - wp)", ORDER, "phase C: the key's x counts the row once too often")
# the strict comparison at its new place, all eight neighbours at once (one at a time: 530 - 537).  Run on the constructed cells alone: of two equal neighbours both then
# survive, and only there is the number of survivors known to stay far below the cell's slots
M(566, F, "keep = s > imax(m0, m1);", "keep = s >= imax(m0, m1);", ORDER[:1], "phase C: a tie with any neighbour survives")

# ---- k_quadtree.hip ------------------------------------------------------------------------------------------------------------------------------------------------
F = "k_quadtree.hip"
QT = EXTRACT + ["test_quadtree_primitives.py", "test_quadtree_gather.py", "test_quadtree_lazy_sort.py"]
M(600, F, "else if (nnodes + nexp * 3 > N) {", "else if (nnodes + nexp * 3 >= N) {", QT, "quadtree: the final rounds begin when a full pass could reach exactly N")
# The child a key falls into (DivideNode :651-661) is spelled once per partition form.  Every mutant below changes count AND placement of one form together (one
# classification feeds both, or both texts are edited), so the keys stay inside the node's span; the forms that the default build reaches only on big dense
# levels are built with ORBX_PRESORT_MAX=1 (every division below depth 1 moves its keys: spans of thousands of keys on a 320 x 256 noise image)
DEEP = ("-DORBX_PRESORT_MAX=1",)
_CLS = "const bool left = key_x(key) < mx, top = key_y(key) < my;"
M(601, F, _CLS + "\n        return left", _CLS.replace("< mx", "<= mx") + "\n        return left", QT, "workgroup partition: a key on the dividing column goes left", defines=DEEP)
M(602, F, _CLS + "\n        return left", _CLS.replace("< my", "<= my") + "\n        return left", QT, "workgroup partition: a key on the dividing row goes up", defines=DEEP)
_C4 = "const bool left = key_x(key[u]) < mx, top = key_y(key[u]) < my;"
M(603, F, _C4, _C4.replace("< mx", "<= mx"), QT, "one-wave partition (<= 256 keys): a key on the dividing column goes left", defines=DEEP)
M(604, F, _C4, _C4.replace("< my", "<= my"), QT, "one-wave partition (<= 256 keys): a key on the dividing row goes up", defines=DEEP)
_W1 = "const uint32_t key = src[s + i0 + lane];\n            " + _CLS
_W2 = "\n            key = src[s + i0 + lane];\n            " + _CLS
M(605, F, _W1, _W1.replace("< mx", "<= mx"), QT, "one-wave partition (> 256 keys): a key on the dividing column goes left", more=[(_W2, _W2.replace("< mx", "<= mx"))], defines=DEEP)
M(606, F, _W1, _W1.replace("< my", "<= my"), QT, "one-wave partition (> 256 keys): a key on the dividing row goes up", more=[(_W2, _W2.replace("< my", "<= my"))], defines=DEEP)
M(607, F, "const bool left = x < mx;", "const bool left = x <= mx;", QT, "presort: a key on a dividing column goes left (bucket table)")
M(608, F, "const bool top = y < my;", "const bool top = y <= my;", QT, "presort: a key on a dividing row goes up (bucket table)")
M(609, F, "if (ds > 0 || ko < bo) { best = key[u];", "if (ds > 0 || ko > bo) { best = key[u];", QT, "final selection: of equal responses the LAST in vKeys order wins (per lane)")
M(610, F, "if (os > bs || (os == bs && oo < bo)) {", "if (os > bs || (os == bs && oo > bo)) {", QT, "final selection: of equal responses the LAST in vKeys order wins (between lanes)")
M(611, F, "if (ds < 0) continue;", "if (ds <= 0) continue;", QT, "final selection: of equal responses the first in buffer order wins, not the first in vKeys order")
M(612, F, "const uint32_t v = best[bk]; w = v > w ? v : w;", "const uint32_t v = best[bk]; w = (v > w) == (w != 0u) ? w : v;", QT, "final selection, never-sorted tree: the smallest bucket word wins")

# ---- libstdcxx_sort_model.h: the pieces k_quadtree.hip runs (median of three, heap fallback; block_sort_libstdcxx has its own range loop) -----------------------------
# Only ties are turned: `!less(b, a)` for `less(a, b)` differs from it on equal keys alone, so the pick is still A median of the three and the unguarded partition
# keeps both its sentinels; the heap's loops are bounded by indices, not by comparisons.  What stays out is in the README, line by line.
F = "libstdcxx_sort_model.h"
SORT = ["test_quadtree_primitives.py"] + EXTRACT
M(650, F, "if (less(a[ia], a[ib])) {", "if (!less(a[ib], a[ia])) {", SORT, "median of three: a == b takes the a < b branch")
M(651, F, "if (less(a[ib], a[ic])) pick = ib;", "if (!less(a[ic], a[ib])) pick = ib;", SORT, "median of three (a < b): b == c picks b, not c")
M(652, F, "else if (less(a[ia], a[ic])) pick = ic;", "else if (!less(a[ic], a[ia])) pick = ic;", SORT, "median of three (a < b, c <= b): a == c picks c, not a")
M(653, F, "} else if (less(a[ia], a[ic])) pick = ia;", "} else if (!less(a[ic], a[ia])) pick = ia;", SORT, "median of three (a >= b): a == c picks a")
M(654, F, "else if (less(a[ib], a[ic])) pick = ic;", "else if (!less(a[ic], a[ib])) pick = ic;", SORT, "median of three (a >= b, a >= c): b == c picks c, not b")
M(655, F, "if (less(a[first + child], a[first + (child - 1)])) child--;", "if (!less(a[first + (child - 1)], a[first + child])) child--;", SORT, "heap fallback: of equal children the left one goes up")
M(656, F, "while (hole > top && less(a[first + parent], value)) {", "while (hole > top && !less(value, a[first + parent])) {", SORT, "heap fallback: a value rises past an equal parent")

# ---- k_image.hip ---------------------------------------------------------------------------------------------------------------------------------------------------
F = "k_image.hip"
_V = "int v = ((mul24_forced(b0, h0 >> 4) >> 16) + (mul24_forced(b1, h1 >> 4) >> 16) + 2) >> 2;"
_V1 = _V.replace("+ 2) >> 2", "+ 1) >> 2")
M(700, F, "a1[k]);\n                " + _V, "a1[k]);\n                " + _V1, IMAGE, "k_resize: rounding term 1")
M(701, F, "a1);\n                " + _V, "a1);\n                " + _V1, IMAGE, "k_pyramid_fused: rounding term 1")
M(702, F, "mulhi_u24_uniform(b1, Hc[k]), 2u);", "mulhi_u24_uniform(b1, Hc[k]), 1u);", IMAGE, "k_resize_rows: rounding term 1")
M(704, F, "a1[k]);\n                " + _V + "\n                v = imin(imax(v, 0), 255);", "a1[k]);\n                " + _V + "\n                v = imin(imax(v, 0), 254);", IMAGE, "k_resize: clamp at 254")
M(705, F, "a1);\n                " + _V + "\n                v = imin(imax(v, 0), 255);", "a1);\n                " + _V + "\n                v = imin(imax(v, 0), 254);", IMAGE, "k_pyramid_fused: clamp at 254")
M(706, F, "H[k] = dot2_u16(byte_perm(w.hi, w.lo, sel[k]), wgt[k], 0u) & ~15u;", "H[k] = dot2_u16(byte_perm(w.hi, w.lo, sel[k]), wgt[k], 0u) & ~7u;", IMAGE, "k_resize_rows: the horizontal sum keeps bit 3")
M(707, F, "p = p < 0 ? -p : 2 * len - 2 - p;", "p = p < 0 ? -p - 1 : 2 * len - 2 - p;", IMAGE, "framed export: left / upper border mirrors with the edge pixel repeated (REFLECT)")
M(708, F, "p = p < 0 ? -p : 2 * len - 2 - p;", "p = p < 0 ? -p : 2 * len - 1 - p;", IMAGE, "framed export: right / lower border mirrors with the edge pixel repeated (REFLECT)")
M(709, F, "a1[k]);\n                " + _V, "a1[k]);\n                " + _V.replace("h0 >> 4", "h0 >> 5"), IMAGE, "k_resize: the upper row's horizontal sum shifted by 5")
M(710, F, "a1[k]);\n                " + _V, "a1[k]);\n                " + _V.replace("h1 >> 4) >> 16", "h1 >> 4) >> 17"), IMAGE, "k_resize: the lower row's product shifted by 17")
M(711, F, "a1);\n                " + _V, "a1);\n                " + _V.replace("h0 >> 4", "h0 >> 5"), IMAGE, "k_pyramid_fused: the upper row's horizontal sum shifted by 5")
M(712, F, "a1);\n                " + _V, "a1);\n                " + _V.replace("h1 >> 4) >> 16", "h1 >> 4) >> 17"), IMAGE, "k_pyramid_fused: the lower row's product shifted by 17")
M(713, F, "b1 = (uint32_t)(ty.w >> 16) << 12;", "b1 = (uint32_t)(ty.w >> 16) << 11;", IMAGE, "k_resize_rows: the lower row's weight scaled by 2^11 (its product shifted by 17)")

# ---- blur_body.h (included by k_image.hip and k_fast.hip) ----------------------------------------------------------------------------------------------------------
F = "blur_body.h"
M(750, F, "if (col < 0) col = -col;", "if (col < 0) col = -col - 1;", IMAGE, "blur: left border mirrors with the edge column repeated")
M(751, F, "if (col >= L.w) col = 2 * L.w - 2 - col;", "if (col >= L.w) col = 2 * L.w - 1 - col;", IMAGE, "blur: right border mirrors with the edge column repeated")
M(752, F, "if (y < 0) y = -y;", "if (y < 0) y = -y - 1;", IMAGE, "blur: upper border mirrors with the edge row repeated")
M(753, F, "if (y >= L.h) y = 2 * L.h - 2 - y;", "if (y >= L.h) y = 2 * L.h - 1 - y;", IMAGE, "blur: lower border mirrors with the edge row repeated")
M(754, F, "dot2_u16(Q[3][j], Ke3, 32768u)", "dot2_u16(Q[3][j], Ke3, 32767u)", IMAGE, "blur: rounding term 32767 (even rows)")
M(755, F, "dot2_u16(Q[3][j], Ko3, 32768u)", "dot2_u16(Q[3][j], Ko3, 32767u)", IMAGE, "blur: rounding term 32767 (odd rows)")
M(756, F, "const bool exact256 = 2 * (k0 + k1 + k2) + k3 <= 256;", "const bool exact256 = 2 * (k0 + k1 + k2) + k3 < 256;", IMAGE, "blur: taps that sum to 256 take the shift-and-clamp form",
  "equivalent: with taps that sum to 256 the accumulator is at most 255 * 65536 + 32768, so `>> 16` is byte 2 and the clamp at 255 never acts: both forms give the same bytes")
M(757, F, "const bool exact256 = 2 * (k0 + k1 + k2) + k3 <= 256;", "const bool exact256 = 2 * (k0 + k1 + k2) + k3 <= 257;", IMAGE, "blur: taps that sum to 257 take the byte-permute form (no clamp)")
M(758, F, "ve = ve > 255u ? 255u : ve;", "ve = ve > 255u ? 254u : ve;", IMAGE, "blur: the clamp of the 257 taps gives 254 (even rows)")
M(759, F, "uint32_t ve = ae[j] >> 16, vo = ao[j] >> 16;", "uint32_t ve = ae[j] >> 15, vo = ao[j] >> 16;", IMAGE, "blur, 257 taps: even rows shifted by 15 (then clamped)")
M(760, F, "oe = byte_perm(ae[1], ae[0], 0x0c0c0602u)", "oe = byte_perm(ae[1], ae[0], 0x0c0c0501u)", IMAGE, "blur, 256 taps: byte 1 of the accumulators of columns 0 and 1, a shift by 8 (even rows)")

# ---- k_input.hip ---------------------------------------------------------------------------------------------------------------------------------------------------
F = "k_input.hip"
M(800, F, "+ p11 * w11 + (1 << 14)) >> 15;", "+ p11 * w11 + (1 << 14) - 1) >> 15;", INPUT, "remap: rounding term one less")
M(801, F, "+ ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;", "+ ((b1 * (h1 >> 4)) >> 16) + 1) >> 2;", INPUT, "input resize: rounding term 1")
M(802, F, "const int half = 1 << (shift - 1);", "const int half = (1 << (shift - 1)) - 1;", INPUT, "grey: rounding term one less")
M(803, F, "r = byte_at(3 * j + ridx);", "r = byte_at(3 * j + 2 - ridx);", INPUT, "grey, 3 channels: red read from the blue channel")
M(804, F, "r = (int)((q >> (8 * ridx)) & 0xFFu);", "r = (int)((q >> (8 * (2 - ridx))) & 0xFFu);", INPUT, "grey, 4 channels: red read from the blue channel")
M(805, F, "(int)q[ridx] * ry", "(int)q[2 - ridx] * ry", INPUT, "grey, partial group: red read from the blue channel")
M(806, F, "fsx = __float2int_rn(__fmul_rn(mx, 32.0f))", "fsx = (int)floorf(__fmul_rn(mx, 32.0f))", INPUT, "remap: x fixed point truncated instead of rounded")
M(807, F, "fsy = __float2int_rn(__fmul_rn(my, 32.0f))", "fsy = (int)floorf(__fmul_rn(my, 32.0f))", INPUT, "remap: y fixed point truncated instead of rounded")
M(808, F, "(((b0 * (h0 >> 4)) >> 16)", "(((b0 * (h0 >> 5)) >> 16)", INPUT, "input resize: the upper row's horizontal sum shifted by 5")

# ---- orbx_api.cpp: the host tables that feed the extraction kernels ------------------------------------------------------------------------------------------------
F = "orbx_api.cpp"
TABLES = EXTRACT + ["test_abi.py"]
M(900, F, "h->quota[l] = round_half_even_f(want);", "h->quota[l] = (int)want;", TABLES, "feature quota per level truncated instead of rounded")
M(901, F, "std::max(h->nfeatures - sum, 0);", "std::max(h->nfeatures - sum - 1, 0);", TABLES, "feature quota: the last level gets one less than the remainder")
M(902, F, "if (iniX >= maxBX - 6) continue;", "if (iniX > maxBX - 6) continue;", TABLES, "cell table: a column that starts at maxBX - 6 is kept",
  "equivalent: such a cell has x0 = iniX + 3 = maxBX - 3 = x1, an empty interior; it takes no slot ((iw + 1) / 2 = 0) and fast_block writes the count 0 for it "
  "(csrc/k_fast.hip: ci.x1 - ci.x0 <= 0), and the candidate lists are read cell by cell")
M(903, F, "L.wcell = (int)ceil(width / L.ncols);", "L.wcell = (int)floor(width / L.ncols);", TABLES, "cell table: cell width rounded down")
M(904, F, "L.hcell = (int)ceil(height / L.nrows);", "L.hcell = (int)floor(height / L.nrows);", TABLES, "cell table: cell height rounded down")
M(905, F, "um[v] = round_half_even_d(sqrt(hp2 - v * v));", "um[v] = (int)sqrt(hp2 - v * v);", TABLES, "umax: half-widths truncated instead of rounded")
M(906, F, "L.w = round_half_even_f((float)W * h->inv_scale[l]);", "L.w = (int)((float)W * h->inv_scale[l]);", TABLES, "level width truncated instead of rounded")
M(907, F, "a1 = round_half_even_f(f * 2048.f);", "a1 = (int)(f * 2048.f);", TABLES + ["test_emu_input.py"], "resize taps: the second weight truncated instead of rounded")
M(908, F, "L.patch = (int)(31 * h->scale[l]);", "L.patch = (int)(31 * h->scale[l] + 0.5f);", TABLES, "keypoint size rounded instead of truncated")
M(909, F, "h->sigma2[i] = h->scale[i] * h->scale[i];", "h->sigma2[i] = h->scale[i];", TABLES, "level sigma2 table: the scale itself")
M(910, F, "h->scale[i] = (float)(h->scale[i - 1] * h->scaleFactor);", "h->scale[i] = (float)pow((double)h->scaleFactor, (double)i);", TABLES, "scale table: the power, not the running product")
M(911, F, "h->inv_scale[i] = 1.0f / h->scale[i];", "h->inv_scale[i] = (float)pow(1.0 / (double)h->scaleFactor, (double)i);", TABLES, "inverse scale table: the power of the inverse factor, not the inverse of the scale")
M(912, F, "h->inv_sigma2[i] = 1.0f / h->sigma2[i];", "h->inv_sigma2[i] = h->inv_scale[i] * h->inv_scale[i];", TABLES, "inverse sigma2 table: the square of the inverse scale")

# ---- orbm_search.cpp: the host replays of the single-frame ORBmatcher entries (ids from 1000) -------------------------------------------------------------------
# The kernels hand back ordered candidate lists; the reference's accept loop is replayed over them on the host.  Host code runs inside the test process like an emulated
# kernel, so the safety rule is the same: no sizes, Packer / Bump / ensure offsets, loop bounds or launch geometry; no guard in front of an index or a write
# (`b.idx >= 0`, `best[k] < 0`, `ltr != -1`, `rtl != -1`, `m12[i] < 0`, `matches12[i1] >= 0` of the prev update, `nleft2 > K2->N`, `N >= 65535`, `it.cnt2 > 0xFFFF`,
# `l < kMaxLevels`, `lvl != -1 && lvl >= 0 && lvl < F->right.nlevels`) removed - the level gates in front of scale_factors[] are only moved inwards; no argument check.
# `rot < 0` is not removed either (a negative bin would index in front of the histogram): it is moved to `rot < -1`, whose bins stay at 0.
F = "orbm_search.cpp"
HG, HR = "test_host_replay_gates.py", "test_host_rotation_gates.py"
H_MAPPTS = [HG, "test_branch_edges_search.py", "test_emu_search.py", "test_local_points.py", "test_search_gates.py"]
H_FRAME = [HG, "test_emu_search.py", "test_lastframe_batch.py", "test_batch_table_forms.py"]
H_SCAN = [HG, "test_emu_search.py", "test_branch_edges_search.py", "test_lastframe_batch.py", "test_branch_edges_windows.py"]
H_ROT = [HR, "test_branch_edges_rotation.py", "test_emu_search.py", "test_lastframe_batch.py"]
H_TRI = [HG, "test_branch_edges_triangulation.py", "test_emu_search.py", "test_keyframe_search_gates.py"]
H_BOW = [HG, "test_emu_search.py", "test_branch_edges_rotation.py", "test_keyframe_search_gates.py", "test_bow_frames_batch.py"]
H_BOWF = [HG, "test_rig_bow_batch.py"]
H_INIT = [HG, "test_branch_edges_search.py", "test_emu_search.py"]
H_PROJ = [HG, "test_emu_search.py", "test_branch_edges_windows.py", "test_lastframe_batch.py", "test_sim3_projection_batch.py"]
H_FISH = [HG, "test_emu_search.py", "test_rig_tracking_batch.py", "test_local_points_rig.py", "test_search_gates.py"]
H_RES = [HR, "test_keyframe_search_gates.py", "test_resident_keyframes.py", "test_branch_edges_rotation.py"]
H_FRUSTUM = ["test_local_points.py", "test_local_points_rig.py", "test_search_gates.py"]
# scan_best / scan_best2
M(1000, F, "if (dist < b.dist) { b.dist = dist; b.idx = idx; }", "if (dist <= b.dist) { b.dist = dist; b.idx = idx; }", H_SCAN, "scan_best: the last of equal distances wins")
M(1001, F, "if (occ && occ[idx + off]) continue;\n        if (dist < b.dist)", "if (dist < b.dist)", H_SCAN, "scan_best: the occupancy skip removed")
M(1002, F, "if (occ && occ[idx + off]) continue;\n        if (dist < b.dist)", "if (occ && occ[idx]) continue;\n        if (dist < b.dist)", H_FISH, "scan_best: camera 2's occupancy read at camera 1's slots")
M(1003, F, "if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestLevel2", "if (dist <= bestDist) { bestDist2 = bestDist; bestDist = dist; bestLevel2", H_MAPPTS, "scan_best2: the last of equal distances wins")
M(1004, F, "else if (dist < bestDist2) { bestLevel2 = level;", "else if (dist <= bestDist2) { bestLevel2 = level;", H_MAPPTS, "scan_best2: a candidate as far as the second best gives it its level")
M(1005, F, "bestLevel2 = bestLevel; bestLevel = level; bestIdx = idx; }", "bestLevel = level; bestIdx = idx; }", H_MAPPTS, "scan_best2: a displaced best does not hand its level to the second")
M(1006, F, "{ bestDist2 = bestDist; bestDist = dist; bestLevel2", "{ bestDist = dist; bestLevel2", H_MAPPTS, "scan_best2: a displaced best does not hand its distance to the second")
M(1007, F, "else if (dist < bestDist2) { bestLevel2 = level; bestDist2 = dist; }", "else if (dist < bestDist2) { bestDist2 = dist; }", H_MAPPTS, "scan_best2: the second best's level not recorded")
M(1008, F, "if (occ && occ[idx + off]) continue;\n        const int dist = c.dist(q, k), level", "const int dist = c.dist(q, k), level", H_MAPPTS, "scan_best2: the occupancy skip removed")
M(1009, F, "if (occ && occ[idx + off]) continue;\n        const int dist = c.dist(q, k), level", "if (occ && occ[idx]) continue;\n        const int dist = c.dist(q, k), level", H_FISH,
  "scan_best2: camera 2's occupancy read at camera 1's slots")
# replay_mappoints
M(1010, F, "if (b.bestDist <= TH_HIGH) {\n            if (b.bestLevel == b.bestLevel2 && b.bestDist > nnratio * b.bestDist2) continue;",
  "if (b.bestDist < TH_HIGH) {\n            if (b.bestLevel == b.bestLevel2 && b.bestDist > nnratio * b.bestDist2) continue;", H_MAPPTS, "replay_mappoints: a best distance of TH_HIGH refused")
M(1011, F, "b.bestDist > nnratio * b.bestDist2) continue;\n            if (b.bestLevel !=", "b.bestDist >= nnratio * b.bestDist2) continue;\n            if (b.bestLevel !=", H_MAPPTS,
  "replay_mappoints: bestDist == nnratio * bestDist2 refused")
M(1012, F, "if (b.bestLevel == b.bestLevel2 && b.bestDist > nnratio * b.bestDist2) continue;\n            if (b.bestLevel !=",
  "if (b.bestDist > nnratio * b.bestDist2) continue;\n            if (b.bestLevel !=", H_MAPPTS, "replay_mappoints: the ratio test also between different levels")
M(1013, F, "|| b.bestDist <= nnratio * b.bestDist2) {\n                assigned[b.bestIdx] = i;\n                occ[b.bestIdx] = has_obs",
  "|| b.bestDist < nnratio * b.bestDist2) {\n                assigned[b.bestIdx] = i;\n                occ[b.bestIdx] = has_obs", H_MAPPTS, "replay_mappoints: the second `if` strict (bestDist == nnratio * bestDist2 on equal levels refused there)")
M(1014, F, "occ[b.bestIdx] = has_obs ? has_obs[i] : 1;", "occ[b.bestIdx] = 1;", H_MAPPTS, "replay_mappoints: a point without observations occupies its keypoint")
# orbm_search_by_projection_mappoints: the skip tests and the window
M(1015, F, "if (!P->in_view[i]) continue;\n        if (far_points", "if (far_points", H_MAPPTS, "SearchByProjection(MapPoints): the mbTrackInView skip removed")
M(1016, F, "P->track_depth[i] > th_far) continue;\n        if (P->is_bad[i]) continue;\n        const int lvl", "P->track_depth[i] >= th_far) continue;\n        if (P->is_bad[i]) continue;\n        const int lvl",
  H_MAPPTS, "SearchByProjection(MapPoints): depth == thFarPoints is far")
M(1017, F, "if (P->is_bad[i]) continue;\n        const int lvl", "const int lvl", H_MAPPTS, "SearchByProjection(MapPoints): the isBad skip removed")
M(1018, F, "q.min_level = lvl - 1; q.max_level = lvl; q.active = 1; q.gate = 1;", "q.min_level = lvl; q.max_level = lvl; q.active = 1; q.gate = 1;", H_MAPPTS,
  "SearchByProjection(MapPoints): the level below the predicted one refused")
M(1019, F, "q.min_level = lvl - 1; q.max_level = lvl; q.active = 1; q.gate = 1;", "q.min_level = lvl - 1; q.max_level = lvl + 1; q.active = 1; q.gate = 1;", H_MAPPTS,
  "SearchByProjection(MapPoints): the level above the predicted one accepted")
# RotHist
M(1020, F, "if (rot < 0.0) rot += 360.0f;", "if (rot <= 0.0) rot += 360.0f;", H_ROT, "rot_bin: rot == 0 goes to 360 (bin 12)")
M(1021, F, "if (rot < 0.0) rot += 360.0f;", "if (rot < -1.0) rot += 360.0f;", H_ROT, "rot_bin: a rot just below 0 is not wrapped (bin 0 for 12)")
M(1022, F, "if (bin == HISTO_LENGTH) bin = 0;", "if (bin == HISTO_LENGTH - 1) bin = 0;", H_ROT, "rot_bin: bin 29 wraps to 0",
  "unreachable, like the line itself: the factor is the reference's 1 / HISTO_LENGTH = 1 / 30 (not HISTO_LENGTH / 360), rot lies in [0, 360], so round(rot / 30) is at most 12 - "
  "neither 29 nor 30 is ever a bin (tests/test_host_rotation_gates.py pins the largest bin, 12, on the oracle)")
M(1023, F, "int bin = (int)round(rot * factor);", "int bin = (int)(rot * factor);", H_ROT, "rot_bin: the bin truncated instead of rounded")
M(1024, F, "if (s > max1) { max3 = max2;", "if (s >= max1) { max3 = max2;", H_ROT, "three_maxima: the later of two equal strongest bins is first")
M(1025, F, "else if (s > max2) { max3 = max2;", "else if (s >= max2) { max3 = max2;", H_ROT, "three_maxima: the later of two equal second bins is second")
M(1026, F, "else if (s > max3) { max3 = s; ind3 = i; }", "else if (s >= max3) { max3 = s; ind3 = i; }", H_ROT, "three_maxima: the later of two equal third bins is third")
M(1027, F, "if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }", "if (max2 <= 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }", H_ROT, "three_maxima: a second bin of exactly 0.1 max1 dropped")
M(1028, F, "else if (max3 < 0.1f * (float)max1) { ind3 = -1; }", "else if (max3 <= 0.1f * (float)max1) { ind3 = -1; }", H_ROT, "three_maxima: a third bin of exactly 0.1 max1 dropped")
M(1029, F, "if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }", "if (max2 < 0.1f * (float)max1) { ind2 = -1; }", H_ROT, "three_maxima: the third bin survives a weak second")
M(1030, F, "if (i == ind1 || i == ind2 || i == ind3) continue;", "if (i == ind1 || i == ind2) continue;", H_ROT, "prune: the third bin is not spared")
M(1031, F, "if (i == ind1 || i == ind2 || i == ind3) continue;", "if (i == ind1 || i == ind3) continue;", H_ROT, "prune: the second bin is not spared")
M(1032, F, "if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }", "if (s > max1) { max2 = max1; max1 = s; ind2 = ind1; ind1 = i; }", H_ROT,
  "three_maxima: a new strongest bin does not push the second down to third")
M(1033, F, "else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }", "else if (s > max2) { max2 = s; ind2 = i; }", H_ROT, "three_maxima: a new second bin does not push the old one down to third")
# orbm_search_by_projection_frame
M(1040, F, "if (u < Cur->min_x || u > Cur->max_x) continue;", "if (u <= Cur->min_x || u > Cur->max_x) continue;", H_FRAME, "SearchByProjection(Frame): u == mnMinX outside")
M(1041, F, "if (u < Cur->min_x || u > Cur->max_x) continue;", "if (u < Cur->min_x || u >= Cur->max_x) continue;", H_FRAME, "SearchByProjection(Frame): u == mnMaxX outside")
M(1042, F, "if (v < Cur->min_y || v > Cur->max_y) continue;", "if (v <= Cur->min_y || v > Cur->max_y) continue;", H_FRAME, "SearchByProjection(Frame): v == mnMinY outside")
M(1043, F, "if (v < Cur->min_y || v > Cur->max_y) continue;", "if (v < Cur->min_y || v >= Cur->max_y) continue;", H_FRAME, "SearchByProjection(Frame): v == mnMaxY outside")
M(1044, F, "if (oct < 0 || oct >= Cur->nlevels) continue;", "if (oct <= 0 || oct >= Cur->nlevels) continue;", H_FRAME, "SearchByProjection(Frame): octave 0 refused")
M(1045, F, "if (oct < 0 || oct >= Cur->nlevels) continue;", "if (oct < 0 || oct >= Cur->nlevels - 1) continue;", H_FRAME, "SearchByProjection(Frame): the last octave refused")
M(1046, F, "if (forward) { q.min_level = oct; q.max_level = -1; }            // :2018", "if (forward) { q.min_level = oct - 1; q.max_level = -1; }            // :2018", H_FRAME,
  "SearchByProjection(Frame), forward: the octave below accepted")
M(1047, F, "\n        else if (backward) { q.min_level = 0; q.max_level = oct; }", "\n        else if (backward) { q.min_level = 0; q.max_level = oct + 1; }", H_FRAME,
  "SearchByProjection(Frame), backward: the octave above accepted")
M(1048, F, "\n        else if (backward) { q.min_level = 0; q.max_level = oct; }", "\n        else if (backward) { q.min_level = 1; q.max_level = oct; }", H_FRAME,
  "SearchByProjection(Frame), backward: octave 0 refused")
M(1049, F, "\n        else { q.min_level = oct - 1; q.max_level = oct + 1; }", "\n        else { q.min_level = oct; q.max_level = oct + 1; }", H_FRAME, "SearchByProjection(Frame), default: the octave below refused")
M(1050, F, "\n        else { q.min_level = oct - 1; q.max_level = oct + 1; }", "\n        else { q.min_level = oct - 1; q.max_level = oct; }", H_FRAME, "SearchByProjection(Frame), default: the octave above refused")
M(1051, F, "if (!Last->valid[i]) continue;\n        const float u = Last->proj_u[i], v = Last->proj_v[i];\n        if (u < Cur->min_x", "const float u = Last->proj_u[i], v = Last->proj_v[i];\n        if (u < Cur->min_x",
  H_FRAME, "SearchByProjection(Frame): the skip of points without map point / outliers / behind the camera removed")
M(1052, F, "if (b.dist <= TH_HIGH) {\n            assigned[b.idx] = i;\n            occ[b.idx] = Last->has_obs", "if (b.dist < TH_HIGH) {\n            assigned[b.idx] = i;\n            occ[b.idx] = Last->has_obs",
  H_FRAME, "SearchByProjection(Frame): a best distance of TH_HIGH refused")
M(1053, F, "occ[b.idx] = Last->has_obs ? Last->has_obs[i] : 1;", "occ[b.idx] = 1;", H_FRAME, "SearchByProjection(Frame): a point without observations occupies its keypoint")
_FRAME_PRUNE = "hist.add(Last->angle[i], Cur->keys_un[b.idx].angle, b.idx);\n        }\n    }\n    if (check_ori) hist.prune([&](int idx) { "
M(1054, F, _FRAME_PRUNE + "assigned[idx] = -2; nmatches--; });", _FRAME_PRUNE + "assigned[idx] = -1; nmatches--; });", H_FRAME + [HR], "SearchByProjection(Frame): the rotation check resets to -1")
M(1055, F, _FRAME_PRUNE + "assigned[idx] = -2; nmatches--; });", _FRAME_PRUNE + "assigned[idx] = -2; });", H_FRAME + [HR], "SearchByProjection(Frame): the rotation check does not reduce the count")
M(1056, F, "if (forward) { q.min_level = oct; q.max_level = -1; }            // :2018", "if (forward && !backward) { q.min_level = oct; q.max_level = -1; }            // :2018", H_FRAME,
  "SearchByProjection(Frame): backward wins when both flags are set")
# search_for_triangulation_impl
M(1060, F, "if (K1->has_map_point && K1->has_map_point[idx1]) continue;\n                const bool stereo1", "if (K1->has_map_point && !K1->has_map_point[idx1]) continue;\n                const bool stereo1",
  H_TRI, "SearchForTriangulation: the features WITH a map point are searched")
M(1061, F, "K1->u_right[idx1] >= 0;\n                if (only_stereo", "K1->u_right[idx1] > 0;\n                if (only_stereo", H_TRI, "SearchForTriangulation: a right coordinate of exactly 0 is monocular")
M(1062, F, "if (only_stereo && !stereo1) continue;", "if (!stereo1) continue;", H_TRI, "SearchForTriangulation: monocular features always skipped")
M(1063, F, "if (only_stereo && !stereo1) continue;", "if (only_stereo && stereo1) continue;", H_TRI, "SearchForTriangulation: bOnlyStereo skips the stereo features")
M(1064, F, "P.only_stereo = only_stereo; P.coarse = coarse; P.th_low = TH_LOW;\n", "P.only_stereo = only_stereo; P.coarse = coarse; P.th_low = TH_LOW - 1;\n", H_TRI, "SearchForTriangulation: TH_LOW - 1 handed to the kernel")
# orbm_search_by_bow_batch
_BOWSKIP = "     // !pMP || pMP->isBad()\n                BowItem it; it.idx1 = base1[p]"
M(1070, F, "!K1->has_map_point[idx1]) continue;" + _BOWSKIP, "K1->has_map_point[idx1]) continue;" + _BOWSKIP, H_BOW, "SearchByBoW: the features WITHOUT a map point are searched")
M(1071, F, "if (taken[idx2] || d < 0) continue;", "if (d < 0) continue;", H_BOW, "SearchByBoW: a target taken by an earlier feature is a candidate again")
M(1072, F, "if (d < bestDist1) { bestDist2 = bestDist1; bestDist1 = d; bestIdx2 = idx2; }", "if (d <= bestDist1) { bestDist2 = bestDist1; bestDist1 = d; bestIdx2 = idx2; }", H_BOW,
  "SearchByBoW: the last of equal distances wins")
M(1073, F, "{ bestDist2 = bestDist1; bestDist1 = d; bestIdx2 = idx2; }", "{ bestDist1 = d; bestIdx2 = idx2; }", H_BOW, "SearchByBoW: a displaced best does not become the second best")
M(1074, F, "(bestDist1 <= TH_LOW) : (bestDist1 < TH_LOW);", "(bestDist1 < TH_LOW) : (bestDist1 < TH_LOW);", H_BOW, "SearchByBoW(KeyFrame, Frame): a best distance of TH_LOW refused")
M(1075, F, "(bestDist1 <= TH_LOW) : (bestDist1 < TH_LOW);", "(bestDist1 <= TH_LOW) : (bestDist1 <= TH_LOW);", H_BOW, "SearchByBoW(KeyFrame, KeyFrame): a best distance of TH_LOW accepted")
M(1076, F, "if (pass && static_cast<float>(bestDist1) < nnratio * static_cast<float>(bestDist2)) {", "if (pass && static_cast<float>(bestDist1) <= nnratio * static_cast<float>(bestDist2)) {", H_BOW,
  "SearchByBoW: bestDist1 == nnratio * bestDist2 accepted")
M(1077, F, "taken[bestIdx2] = 1;", "taken[bestIdx2] = 0;", H_BOW, "SearchByBoW: a matched target is not marked as taken")
M(1078, F, "if (taken[idx2] || d < 0) continue;", "if (taken[idx2] || d <= 0) continue;", H_BOW, "SearchByBoW: a target at distance 0 skipped like an ineligible one")
M(1079, F, "else if (d < bestDist2) bestDist2 = d;\n            }\n            const bool pass", "else if (d <= bestDist2) bestDist2 = d;\n            }\n            const bool pass", H_BOW,
  "SearchByBoW: second best inclusive", "equivalent: with d == bestDist2 the assignment writes the value that is there")
# orbm_search_by_bow_fisheye
M(1080, F, "if (assigned2[idx2] >= 0) continue;", "if (assigned2[idx2] > 0) continue;", H_BOWF, "SearchByBoW, rig frame: a frame feature taken by key-frame feature 0 is a candidate again")
M(1081, F, "if (idx2 < nleft2) {", "if (idx2 <= nleft2) {", H_BOWF, "SearchByBoW, rig frame: the first feature of camera 2 counts as camera 1's")
M(1082, F, "if (d < bestDist1) { bestDist2 = bestDist1; bestDist1 = d; bestIdxF = idx2; }", "if (d <= bestDist1) { bestDist2 = bestDist1; bestDist1 = d; bestIdxF = idx2; }", H_BOWF,
  "SearchByBoW, rig frame: the last of equal camera-1 distances wins")
M(1083, F, "if (d < bestDist1R) {", "if (d <= bestDist1R) {", H_BOWF, "SearchByBoW, rig frame: the last of equal camera-2 distances wins")
M(1084, F, "if (bestDist1 <= TH_LOW) {\n                if (static_cast<float>(bestDist1) < nnratio", "if (bestDist1 < TH_LOW) {\n                if (static_cast<float>(bestDist1) < nnratio", H_BOWF,
  "SearchByBoW, rig frame: a camera-1 best of TH_LOW refused")
M(1085, F, "< nnratio * static_cast<float>(bestDist2)) {\n                    assigned2[bestIdxF]", "<= nnratio * static_cast<float>(bestDist2)) {\n                    assigned2[bestIdxF]", H_BOWF,
  "SearchByBoW, rig frame: bestDist1 == nnratio * bestDist2 accepted")
M(1086, F, "if (bestDist1R <= TH_LOW) {", "if (bestDist1R < TH_LOW) {", H_BOWF, "SearchByBoW, rig frame: a camera-2 best of TH_LOW refused")
M(1087, F, "if (bestDist1R <= TH_LOW) {", "if (bestDist1R <= TH_LOW && static_cast<float>(bestDist1R) < nnratio * static_cast<float>(bestDist2R)) {", H_BOWF,
  "SearchByBoW, rig frame: the camera-2 match takes a ratio test")
M(1088, F, "if (bestDist1 <= TH_LOW) {\n                if (static_cast<float>(bestDist1) < nnratio", "if (bestDist1 <= TH_LOW || bestDist1R <= TH_LOW) {\n                if (static_cast<float>(bestDist1) < nnratio", H_BOWF,
  "SearchByBoW, rig frame: the camera-2 match is taken without a camera-1 best under TH_LOW")
M(1089, F, "else if (d < bestDist2) bestDist2 = d;\n                } else {", "else if (d < bestDist2) {}\n                } else {", H_BOWF, "SearchByBoW, rig frame: camera 1's second best only from displaced bests")
# orbm_search_for_initialization
M(1090, F, "if (level1 > 0) continue;", "if (level1 > 1) continue;", H_INIT, "SearchForInitialization: level-1 keypoints searched too")
M(1091, F, "if (matched_dist[i2] <= dist) continue;", "if (matched_dist[i2] < dist) continue;", H_INIT, "SearchForInitialization: a keypoint matched at the same distance is a candidate")
M(1092, F, "if (matched_dist[i2] <= dist) continue;", "", H_INIT, "SearchForInitialization: the matched-distance skip removed")
M(1093, F, "if (dist < bestDist) { bestDist2 = bestDist; bestDist = dist; bestIdx2 = i2; }", "if (dist <= bestDist) { bestDist2 = bestDist; bestDist = dist; bestIdx2 = i2; }", H_INIT,
  "SearchForInitialization: the last of equal distances wins")
M(1094, F, "if (bestDist <= TH_LOW) {\n            if (bestDist < (float)bestDist2 * nnratio) {", "if (bestDist < TH_LOW) {\n            if (bestDist < (float)bestDist2 * nnratio) {", H_INIT,
  "SearchForInitialization: a best distance of TH_LOW refused")
M(1095, F, "if (bestDist < (float)bestDist2 * nnratio) {", "if (bestDist <= (float)bestDist2 * nnratio) {", H_INIT, "SearchForInitialization: bestDist == bestDist2 * nnratio accepted")
M(1096, F, "{ matches12[matches21[bestIdx2]] = -1; nmatches--; }", "{ matches12[matches21[bestIdx2]] = -1; }", H_INIT, "SearchForInitialization: a displaced match stays in the count")
M(1097, F, "{ matches12[matches21[bestIdx2]] = -1; nmatches--; }", "{ nmatches--; }", H_INIT, "SearchForInitialization: a displaced match stays in vnMatches12")
M(1098, F, "if (matches21[bestIdx2] >= 0) {", "if (matches21[bestIdx2] > 0) {", H_INIT, "SearchForInitialization: an earlier match by keypoint 0 is not displaced")
M(1099, F, "matches21[bestIdx2] = i1; matched_dist[bestIdx2] = bestDist;", "matches21[bestIdx2] = i1;", H_INIT, "SearchForInitialization: the matched distance not recorded")
M(1100, F, "if (matches12[idx1] >= 0) { matches12[idx1] = -1; nmatches--; }", "{ matches12[idx1] = -1; nmatches--; }", H_INIT + [HR],
  "SearchForInitialization: the rotation check counts a displaced match down again")
M(1101, F, "{ bestDist2 = bestDist; bestDist = dist; bestIdx2 = i2; }", "{ bestDist = dist; bestIdx2 = i2; }", H_INIT, "SearchForInitialization: a displaced best does not become the second best")
# projected_candidates and the four searches on it
M(1110, F, "if (!P->valid[i]) continue;\n        const int lvl = P->pred_level[i];", "const int lvl = P->pred_level[i];", H_PROJ, "projected_candidates: invalid points searched")
M(1111, F, "if (lvl < 0 || lvl >= F->nlevels) continue;\n        q.x = P->u[i];", "if (lvl <= 0 || lvl >= F->nlevels) continue;\n        q.x = P->u[i];", H_PROJ, "projected_candidates: predicted level 0 refused")
M(1112, F, "if (lvl < 0 || lvl >= F->nlevels) continue;\n        q.x = P->u[i];", "if (lvl < 0 || lvl >= F->nlevels - 1) continue;\n        q.x = P->u[i];", H_PROJ, "projected_candidates: the last predicted level refused")
M(1113, F, "q.min_level = lvl - 1; q.max_level = lvl + hi;", "q.min_level = lvl; q.max_level = lvl + hi;", H_PROJ, "projected_candidates: the level below the predicted one refused")
M(1114, F, "q.min_level = lvl - 1; q.max_level = lvl + hi;", "q.min_level = lvl - 1; q.max_level = lvl + hi + 1;", H_PROJ, "projected_candidates: one level more above the predicted one")
M(1120, F, "b.dist <= TH_LOW * ratio_hamming) {", "b.dist < TH_LOW * ratio_hamming) {", H_PROJ, "SearchByProjection(Sim3): a best distance of TH_LOW * ratioHamming refused")
M(1121, F, "{ assigned[b.idx] = i; occ[b.idx] = 1; nmatches++; }", "{ assigned[b.idx] = i; occ[b.idx] = 0; nmatches++; }", H_PROJ, "SearchByProjection(Sim3): a matched keypoint stays free")
M(1122, F, "projected_candidates(h, KF, P, th, 0, 0, nullptr, &qs, &c); if (rc) return rc;\n    const int N = KF->N;", "projected_candidates(h, KF, P, th, 1, 0, nullptr, &qs, &c); if (rc) return rc;\n    const int N = KF->N;",
  H_PROJ, "SearchByProjection(Sim3): the level above the predicted one accepted")
M(1125, F, "b.dist <= orb_dist) {", "b.dist < orb_dist) {", H_PROJ, "SearchByProjection(KeyFrame): a best distance of ORBdist refused")
M(1126, F, "assigned[b.idx] = i; occ[b.idx] = 1; nmatches++;\n", "assigned[b.idx] = i; occ[b.idx] = 0; nmatches++;\n", H_PROJ, "SearchByProjection(KeyFrame): a matched keypoint stays free")
_KF_PRUNE = "hist.add(P->angle[i], Cur->keys_un[b.idx].angle, b.idx);\n        }\n    }\n    if (check_ori) hist.prune([&](int idx) { "
M(1127, F, _KF_PRUNE + "assigned[idx] = -2; nmatches--; });", _KF_PRUNE + "assigned[idx] = -1; nmatches--; });", H_PROJ + [HR], "SearchByProjection(KeyFrame): the rotation check resets to -1")
M(1128, F, "projected_candidates(h, Cur, P, th, 1, 0, nullptr, &qs, &c);", "projected_candidates(h, Cur, P, th, 0, 0, nullptr, &qs, &c);", H_PROJ, "SearchByProjection(KeyFrame): the level above the predicted one refused")
M(1130, F, "b.dist > TH_LOW ? -1 : b.idx;", "b.dist >= TH_LOW ? -1 : b.idx;", H_PROJ + ["test_projection_gates.py"], "Fuse candidates: a best distance of TH_LOW refused")
M(1135, F, "if (b.dist <= TH_HIGH) out[i] = b.idx;", "if (b.dist < TH_HIGH) out[i] = b.idx;", H_PROJ, "SearchBySim3: a best distance of TH_HIGH refused")
M(1136, F, "if (idx2 >= 0 && vnMatch2[idx2] == i1) {", "if (idx2 >= 0) {", H_PROJ, "SearchBySim3: the mutual-agreement test removed")
# the fisheye replays
M(1140, F, "if (!inl && !inr) continue;", "if (!inl) continue;", H_FISH, "SearchByProjection(MapPoints), rig: a point only camera 2 sees is skipped")
M(1141, F, "P->track_depth[i] > th_far) continue;\n        if (P->is_bad[i]) continue;\n        alive[i] = 1;", "P->track_depth[i] >= th_far) continue;\n        if (P->is_bad[i]) continue;\n        alive[i] = 1;",
  H_FISH, "SearchByProjection(MapPoints), rig: depth == thFarPoints is far")
M(1142, F, "if (P->is_bad[i]) continue;\n        alive[i] = 1;", "alive[i] = 1;", H_FISH, "SearchByProjection(MapPoints), rig: the isBad skip removed")
M(1143, F, "const float r = PR->view_cos_r[i] > 0.998 ? 2.5f : 4.0f;", "const float r = PR->view_cos_r[i] > 0.99 ? 2.5f : 4.0f;", H_FISH, "SearchByProjection(MapPoints), rig: camera 2's RadiusByViewingCos at 0.99")
M(1144, F, "float r = P->view_cos[i] > 0.998 ? 2.5f : 4.0f;\n                if (bFactor) r *= th;\n                AreaQuery& q = ql[i];",
  "float r = P->view_cos[i] > 0.99 ? 2.5f : 4.0f;\n                if (bFactor) r *= th;\n                AreaQuery& q = ql[i];", H_FISH, "SearchByProjection(MapPoints), rig: camera 1's RadiusByViewingCos at 0.99")
M(1145, F, "b.bestDist > nnratio * b.bestDist2) skip_right = true;", "b.bestDist > nnratio * b.bestDist2) skip_right = false;", H_FISH,
  "SearchByProjection(MapPoints), rig: camera 2 is searched after camera 1's ratio test failed")
M(1146, F, "if (b.bestDist <= TH_HIGH) {\n                if (b.bestLevel == b.bestLevel2 && b.bestDist > nnratio * b.bestDist2) skip_right",
  "if (b.bestDist < TH_HIGH) {\n                if (b.bestLevel == b.bestLevel2 && b.bestDist > nnratio * b.bestDist2) skip_right", H_FISH, "SearchByProjection(MapPoints), rig: a camera-1 best of TH_HIGH refused")
M(1147, F, "b.bestDist > nnratio * b.bestDist2) skip_right = true;", "b.bestDist >= nnratio * b.bestDist2) skip_right = true;", H_FISH,
  "SearchByProjection(MapPoints), rig: camera 1's bestDist == nnratio * bestDist2 refused")
M(1148, F, "occ[ltr + NL] = obs; nmatches++; }", "occ[ltr + NL] = obs; }", H_FISH, "SearchByProjection(MapPoints), rig: the lapping twin of a camera-1 match is not counted")
M(1149, F, "if (b.bestDist <= TH_HIGH) {\n                if (b.bestLevel == b.bestLevel2 && b.bestDist > nnratio * b.bestDist2) continue;\n                const int rtl",
  "if (b.bestDist < TH_HIGH) {\n                if (b.bestLevel == b.bestLevel2 && b.bestDist > nnratio * b.bestDist2) continue;\n                const int rtl", H_FISH,
  "SearchByProjection(MapPoints), rig: a camera-2 best of TH_HIGH refused")
M(1150, F, "b.bestDist > nnratio * b.bestDist2) continue;\n                const int rtl", "b.bestDist >= nnratio * b.bestDist2) continue;\n                const int rtl", H_FISH,
  "SearchByProjection(MapPoints), rig: camera 2's bestDist == nnratio * bestDist2 refused")
M(1151, F, "if (b.bestLevel == b.bestLevel2 && b.bestDist > nnratio * b.bestDist2) continue;\n                const int rtl", "if (b.bestDist > nnratio * b.bestDist2) continue;\n                const int rtl", H_FISH,
  "SearchByProjection(MapPoints), rig: camera 2's ratio test also between different levels")
M(1152, F, "occ[b.bestIdx] = obs;\n                    const int ltr", "occ[b.bestIdx] = 1;\n                    const int ltr", H_FISH, "SearchByProjection(MapPoints), rig: a point without observations occupies its camera-1 keypoint")
M(1153, F, "occ[rtl] = obs; nmatches++; }", "occ[rtl] = obs; }", H_FISH, "SearchByProjection(MapPoints), rig: the lapping twin of a camera-2 match is not counted")
M(1154, F, "scan_best2(cr, i, occ.data(), NL);", "scan_best2(cr, i, occ.data(), 0);", H_FISH, "SearchByProjection(MapPoints), rig: camera 2's occupancy read without the Nleft offset")
M(1155, F, "|| b.bestDist <= nnratio * b.bestDist2) {\n                    assigned[b.bestIdx] = i; occ[b.bestIdx] = obs;", "|| b.bestDist < nnratio * b.bestDist2) {\n                    assigned[b.bestIdx] = i; occ[b.bestIdx] = obs;",
  H_FISH, "SearchByProjection(MapPoints), rig: camera 1's second `if` strict")
M(1160, F, "if (u < Cur->left.min_x || u > Cur->left.max_x) continue;", "if (u <= Cur->left.min_x || u > Cur->left.max_x) continue;", H_FISH, "SearchByProjection(Frame), rig: u == mnMinX outside")
M(1161, F, "if (u < Cur->left.min_x || u > Cur->left.max_x) continue;", "if (u < Cur->left.min_x || u >= Cur->left.max_x) continue;", H_FISH, "SearchByProjection(Frame), rig: u == mnMaxX outside")
M(1162, F, "if (v < Cur->left.min_y || v > Cur->left.max_y) continue;", "if (v <= Cur->left.min_y || v > Cur->left.max_y) continue;", H_FISH, "SearchByProjection(Frame), rig: v == mnMinY outside")
M(1163, F, "if (v < Cur->left.min_y || v > Cur->left.max_y) continue;", "if (v < Cur->left.min_y || v >= Cur->left.max_y) continue;", H_FISH, "SearchByProjection(Frame), rig: v == mnMaxY outside")
M(1164, F, "if (bl.dist <= TH_HIGH) {", "if (bl.dist < TH_HIGH) {", H_FISH, "SearchByProjection(Frame), rig: a camera-1 best of TH_HIGH refused")
M(1165, F, "if (br.dist <= TH_HIGH) {", "if (br.dist < TH_HIGH) {", H_FISH, "SearchByProjection(Frame), rig: a camera-2 best of TH_HIGH refused")
M(1166, F, "scan_best(cr, i, occ.data(), NL);", "scan_best(cr, i, occ.data(), 0);", H_FISH, "SearchByProjection(Frame), rig: camera 2's occupancy read without the Nleft offset")
M(1167, F, "if (!ql[i].active || cl.count[i] == 0) continue;                   // an empty left", "if (!ql[i].active) continue;                   // an empty left", H_FISH,
  "SearchByProjection(Frame), rig: camera 2 is searched after an empty camera-1 window")
M(1168, F, "\n            if (forward) { q.min_level = oct; q.max_level = -1; }", "\n            if (forward) { q.min_level = oct - 1; q.max_level = -1; }", H_FISH, "SearchByProjection(Frame), rig, forward: the octave below accepted")
M(1169, F, "\n            else if (backward) { q.min_level = 0; q.max_level = oct; }", "\n            else if (backward) { q.min_level = 0; q.max_level = oct + 1; }", H_FISH,
  "SearchByProjection(Frame), rig, backward: the octave above accepted")
M(1170, F, "\n            else { q.min_level = oct - 1; q.max_level = oct + 1; }", "\n            else { q.min_level = oct; q.max_level = oct + 1; }", H_FISH, "SearchByProjection(Frame), rig, default: the octave below refused")
M(1171, F, "br.idx + NL);\n        }\n    }\n    if (check_ori) hist.prune([&](int idx) { assigned[idx] = -2;", "br.idx + NL);\n        }\n    }\n    if (check_ori) hist.prune([&](int idx) { assigned[idx] = -1;",
  H_FISH + [HR], "SearchByProjection(Frame), rig: the rotation check resets to -1")
M(1172, F, "const uint8_t obs = Last->has_obs ? Last->has_obs[i] : 1;\n        const Best bl", "const uint8_t obs = 1;\n        const Best bl", H_FISH,
  "SearchByProjection(Frame), rig: a point without observations occupies its keypoints")
M(1173, F, "\n            else { q.min_level = oct - 1; q.max_level = oct + 1; }", "\n            else { q.min_level = oct - 1; q.max_level = oct; }", H_FISH, "SearchByProjection(Frame), rig, default: the octave above refused")
# prune_by_rotation, fill_frustum_params, right_camera_params
M(1180, F, "hist.add(K1->angle[i], K2->angle[m12[i]], i);", "hist.add(K2->angle[m12[i]], K1->angle[i], i);", H_RES, "prune_by_rotation: the angle difference taken the other way round")
M(1181, F, "m12[idx1] = -1; nmatches--; });\n    return nmatches;", "m12[idx1] = -1; });\n    return nmatches;", H_RES, "prune_by_rotation: the rotation check does not reduce the count")
M(1185, F, "Fp->kb8 = V->camera_type == 1;", "Fp->kb8 = V->camera_type != 1;", H_FRUSTUM, "fill_frustum_params: the camera models swapped")
M(1186, F, "R.camera_type = V->camera2_type;", "R.camera_type = V->left.camera_type;", [HG] + H_FRUSTUM[1:], "right_camera_params: camera 2 takes camera 1's model",
  "no reference answer where it differs: both cameras of a Frame with Nleft != -1 are KannalaBrandt8 in the reference (the two-camera constructor, src/Frame.cc:1432, is called where Tracking holds an mpCamera2, and that is "
  "only ever a `new KannalaBrandt8`, src/Tracking.cc:1132, beside a fisheye first camera), every rig of the suite and of the reference drivers (oracle/ref_frame_driver.cpp) is such a pair, and with equal models the mutant "
  "computes the same; a pinhole camera beside a fisheye one would have nothing to be compared with")
M(1187, F, "Fp->rig_mode = 1;", "Fp->rig_mode = 0;", [HG] + H_FRUSTUM[1:], "right_camera_params: camera 2 judged in the single-camera mode")

# ---- the drop-in facade headers (ids from 2000) -----------------------------------------------------------------------------------------------------------------
# A file named from the repository root (include/orb_slam3_amd/...): the tool edits a copy of include/, builds oracle/_ref/libmw_facade*.so from the copy where the
# mutant's tests load them, and leaves the emulator library alone.  tests/test_callers_compile.py never stands in a group: it reads objects made from the real headers.
# The safety rule is the host code's - a mutant runs inside the test drivers, on the emulator, in host memory:
#   no sizes, no `M > 0 ? M : 1` buffers, no loop bounds;
#   no guard removed in front of an index or a dereference (`!pMP`, `!incoming`, `!p`, `points[i] &&`, `best[i] < 0`, `m12[i] >= 0`, `assigned[i] >= 0`,
#   `j >= 0 && j < n[1]`, `row < 0`, `k < (int)rowOf.size()`, `it == mAdds.end()`, `v_ == nullptr ||`, `(int)vpMatched.size() != pKF->N`, `mpCamera2 &&` in front of
#   mpCamera2->, `u_right = nullptr` under mpCamera2: a rig's mvuRight holds Nleft values and the device would read N);
#   no Check(...) removed; nothing that destroys a device object twice or uses one after its destroy (Adopt's `dev != dev` test may only be mutated towards a leak,
#   the transient rule only towards caching, FuseBatch::Add's own upload of a key frame without BoW not at all: through Get it would be the transient, destroyed by
#   the next Get of the same call).  A mutant that leaks is allowed: the library's live count shows it.  `crashed` fails the pass.
FH = "include/orb_slam3_amd/ORBmatcher.h"
FG = "test_facade_gates.py"                                           # the new files: the mock-type driver (cache, FuseBatch, Fuse) and the constructed database
KG = "test_kfdb_gates.py"
MG = "test_matcher_gates.py"                                          # ... and the hand-built `gates` worlds of tests/matcher_world.py, through the reference and the facade
MOCK = "test_facade.py::test_matcher_facade_emulated"
MWREF = "test_matcher_reference.py::test_matcher_facade_equals_reference_emulated"
MWFUZZ = "test_matcher_reference.py::test_matcher_facade_equals_reference_random_parameters_emulated"
F_MW = [MG, FG, MOCK, MWREF, MWFUZZ]
F_FUSE = [MG, FG, "test_fuse_many_facade.py", MOCK, MWREF]
F_SIM3 = [MG, FG, "test_sim3_many_facade.py", MWREF]
F_CACHE = [FG, "test_keyframe_extracted.py::test_facade_adopt", "test_fuse_many_facade.py", MOCK, "test_shared_objects.py::test_resident_keyframes_shared_by_threads_emulated",
           "test_lifetime.py::test_facade_worlds_leave_nothing_behind", MWREF]
F_KFDB = [KG, "test_kfdb_facade.py"]
F_EXTRACT = ["test_facade.py::test_facade_dropin_emulated", "test_pyramid_export_facade.py", "test_mono_init.py::test_facade_constructs_every_mono_init_extractor_emulated"]
F_VOC = ["test_facade.py::test_vocabulary_facade_emulated", "test_shared_objects.py::test_vocabulary_facade_shared_by_threads_emulated"]
TWICE = ("equivalent: Fuse tests the point twice on purpose - the head only chooses what is projected, and the replay loop reads isBad / IsInKeyFrame again before anything is written; "
         "a point that the head lets through wrongly is projected, searched and then skipped there")
ROUTE = "equivalent in the result: the condition only chooses between the resident and the uploaded form of the same search, which tests/test_resident_keyframes.py holds equal"
# SearchByProjection(Frame, MapPoints)
M(2000, FH, "hasObs[i] = p->Observations() > 0;", "hasObs[i] = p->Observations() >= 0;", F_MW, "SearchByProjection(MapPoints): a point without observations counts as observed")
M(2001, FH, "bad[i] = p->isBad(); hasObs[i]", "bad[i] = 0; hasObs[i]", F_MW, "SearchByProjection(MapPoints): isBad not read")
M(2002, FH, "inViewR[i] = p->mbTrackInViewR;", "inViewR[i] = p->mbTrackInView;", F_MW, "SearchByProjection(MapPoints), rig: camera 2 takes camera 1's mbTrackInView")
M(2003, FH, "FillFrame(F, fs, OccupiedWithObservations);", "FillFrame(F, fs, OccupiedAny);", F_MW, "SearchByProjection(MapPoints): a keypoint with an unobserved point is occupied")
M(2004, FH, "FillRig(F, rs, OccupiedWithObservations);", "FillRig(F, rs, OccupiedAny);", F_MW, "SearchByProjection(MapPoints), rig: a keypoint with an unobserved point is occupied")
# SearchByProjection(Frame, LastFrame)
M(2010, FH, "zLastOfCurCentre > CurrentFrame.mb, away", "zLastOfCurCentre >= CurrentFrame.mb, away", F_MW, "SearchByProjection(LastFrame): z == mb is `towards`")
M(2011, FH, "-zLastOfCurCentre > CurrentFrame.mb;", "-zLastOfCurCentre >= CurrentFrame.mb;", F_MW, "SearchByProjection(LastFrame): -z == mb is `away`")
M(2012, FH, "towards = !bMono && zLastOfCurCentre", "towards = zLastOfCurCentre", F_MW, "SearchByProjection(LastFrame): bMono does not switch `towards` off")
M(2013, FH, "away = !bMono && -zLastOfCurCentre", "away = -zLastOfCurCentre", F_MW, "SearchByProjection(LastFrame): bMono does not switch `away` off")
M(2014, FH, "if (!pMP || LastFrame.mvbOutlier[i]) continue;", "if (!pMP) continue;", F_MW, "SearchByProjection(LastFrame): outliers are searched")
M(2015, FH, "seen[i] = pMP->Observations() > 0;", "seen[i] = 1;", F_MW, "SearchByProjection(LastFrame): a point without observations occupies its keypoint")
M(2016, FH, "FillFrame(CurrentFrame, fs, OccupiedWithObservations);", "FillFrame(CurrentFrame, fs, OccupiedAny);", F_MW, "SearchByProjection(LastFrame): a keypoint with an unobserved point is occupied")
M(2017, FH, "FillRig(CurrentFrame, rs, OccupiedWithObservations);", "FillRig(CurrentFrame, rs, OccupiedAny);", F_MW, "SearchByProjection(LastFrame), rig: a keypoint with an unobserved point is occupied")
M(2018, FH, "CurrentFrame.mvpMapPoints[i] = LastFrame.mvpMapPoints[assigned[i]];\n            else if (assigned[i] == -2) CurrentFrame.mvpMapPoints[i] = nullptr;",
  "CurrentFrame.mvpMapPoints[i] = LastFrame.mvpMapPoints[assigned[i]];", F_MW, "SearchByProjection(LastFrame): a match that the rotation check removes leaves the keypoint's old point")
M(2019, FH, "right.depth_test = 0; right.bounds_mode = 2;", "right.depth_test = 2; right.bounds_mode = 2;", F_MW, "SearchByProjection(LastFrame), rig: camera 2's projection takes a depth test")
M(2020, FH, "spec.depth_test = 2;                                  // 1 / z < 0 rejects", "spec.depth_test = 1;                                  // 1 / z < 0 rejects", F_MW,
  "SearchByProjection(LastFrame): the depth test of the other methods (z <= 0)")
# SearchByProjection(Frame, KeyFrame, sAlreadyFound)
M(2025, FH, "if (pMP && !pMP->isBad() && !sAlreadyFound.count(pMP)) pts.take(i, pMP, false);", "if (pMP && !sAlreadyFound.count(pMP)) pts.take(i, pMP, false);", F_MW,
  "SearchByProjection(KeyFrame): bad points are searched")
M(2026, FH, "if (pMP && !pMP->isBad() && !sAlreadyFound.count(pMP)) pts.take(i, pMP, false);", "if (pMP && !pMP->isBad()) pts.take(i, pMP, false);", F_MW,
  "SearchByProjection(KeyFrame): points already found are searched")
M(2027, FH, "FillFrame(CurrentFrame, fs, OccupiedAny);", "FillFrame(CurrentFrame, fs, OccupiedWithObservations);", F_MW, "SearchByProjection(KeyFrame): a keypoint with an unobserved point is free")
M(2028, FH, "CurrentFrame.mvpMapPoints[i] = kfPoints[assigned[i]];\n            else if (assigned[i] == -2) CurrentFrame.mvpMapPoints[i] = nullptr;", "CurrentFrame.mvpMapPoints[i] = kfPoints[assigned[i]];", F_MW,
  "SearchByProjection(KeyFrame): the -2 -> nullptr write-back removed",
  "equivalent: under OccupiedAny only a keypoint that was NULL on entry can be matched, so a match that the rotation check removes (-2) leaves what was there, NULL, with or without the line")
M(2029, FH, "spec.distance_test = 1;                               // no depth test", "spec.distance_test = 0;                               // no depth test", F_MW,
  "SearchByProjection(KeyFrame): the distance-range test switched off")
# the Sim3 projection searches, single and many
M(2030, FH, "if (!pMP->isBad() && !taken.count(pMP)) pts.take(i, pMP, true);", "if (!taken.count(pMP)) pts.take(i, pMP, true);", F_SIM3 + [MWFUZZ], "SearchByProjection(Sim3): bad points are searched")
M(2031, FH, "if (!pMP->isBad() && !taken.count(pMP)) pts.take(i, pMP, true);", "if (!pMP->isBad()) pts.take(i, pMP, true);", F_SIM3 + [MWFUZZ], "SearchByProjection(Sim3): points already matched are searched")
M(2033, FH, "for (int i = 0; i < N; i++) fs.occ[i] = vpMatched[i] != nullptr;", "for (int i = 0; i < N; i++) fs.occ[i] = 0;", F_SIM3 + [MWFUZZ], "SearchByProjection(Sim3): matched keypoints are free")
M(2034, FH, "if (inlineProjection) { spec.camera_type = 0;", "if (!inlineProjection) { spec.camera_type = 0;", F_SIM3 + [MWFUZZ], "Sim3ProjectionSpec: the two overloads' projections swapped")
M(2035, FH, "spec.inline_pinhole = 1; }", "spec.inline_pinhole = 0; }", F_SIM3 + [MWFUZZ], "Sim3ProjectionSpec: the inline form projects like GeometricCamera::project")
M(2036, FH, "spec.depth_test = 1; spec.distance_test = 1; spec.angle_test = 1;\n        return spec;", "spec.depth_test = 1; spec.distance_test = 1; spec.angle_test = 0;\n        return spec;", F_SIM3 + [MWFUZZ],
  "Sim3ProjectionSpec: the viewing-angle test switched off")
M(2037, FH, "return SE3T(S.rotationMatrix(), S.translation() / S.scale());", "return SE3T(S.rotationMatrix(), S.translation());", F_SIM3 + F_FUSE[1:], "RigidPart: the translation is not divided by the scale")
M(2038, FH, "{ vpMatched[idx] = vpPoints[assigned[idx]]; vpMatchedKF[idx] = vpPointsKFs[assigned[idx]]; }", "{ vpMatched[idx] = vpPoints[assigned[idx]]; }", F_SIM3 + [MWFUZZ],
  "SearchByProjection(Sim3, vpPointsKFs): vpMatchedKF not written")
M(2039, FH, "if (pKF->NLeft != -1 || (int)vpMatched.size() != pKF->N) continue;", "if ((int)vpMatched.size() != pKF->N) continue;", F_SIM3, "SearchByProjection(Sim3), many: a rig key frame takes the batched route")
M(2040, FH, "return !p || p->isBad() || taken[row].count(p) != 0; }", "return !p || taken[row].count(p) != 0; }", F_SIM3, "SearchByProjection(Sim3), many: bad points are searched")
M(2041, FH, "return !p || p->isBad() || taken[row].count(p) != 0; }", "return !p || p->isBad(); }", F_SIM3, "SearchByProjection(Sim3), many: points already matched are searched")
M(2042, FH, "occupied.back()[i] = vpMatched[i] != nullptr;", "occupied.back()[i] = 0;", F_SIM3, "SearchByProjection(Sim3), many: matched keypoints are free")
M(2043, FH, "s.s2 = x.scale(); s.second = 1;", "s.s2 = x.scale(); s.second = 2;", F_MW, "SecondQuaternion: a Sim3 applied as an SE3")
M(2044, FH, "s.s2 = 1.0f; s.second = 2;", "s.s2 = 1.0f; s.second = 1;", F_MW, "SecondQuaternion: an SE3 applied as a Sim3")
# SearchByBoW
M(2045, FH, "if (F.Nleft == -1 && !pKF->mpCamera2 && !pKF->mFeatVec.empty()) {", "if (F.Nleft == -1 && !pKF->mpCamera2) {", F_MW + F_CACHE[1:2], "SearchByBoW(KeyFrame, Frame): a key frame without BoW takes the resident route", ROUTE)
M(2046, FH, "if (F.Nleft == -1 && !pKF->mpCamera2 && !pKF->mFeatVec.empty()) {", "if (!pKF->mpCamera2 && !pKF->mFeatVec.empty()) {", F_MW, "SearchByBoW(KeyFrame, Frame): a rig frame takes the resident route")
M(2047, FH, "if (F.Nleft == -1 && !pKF->mpCamera2 && !pKF->mFeatVec.empty()) {", "if (F.Nleft == -1 && !pKF->mFeatVec.empty()) {", F_MW, "SearchByBoW(KeyFrame, Frame): a rig key frame takes the resident route")
M(2048, FH, "k1.present[i] = vpMapPointsKF[i] && !vpMapPointsKF[i]->isBad();", "k1.present[i] = vpMapPointsKF[i] != nullptr;", F_MW, "SearchByBoW(KeyFrame, Frame), uploaded form: bad points take part")
M(2049, FH, "good[i][j] = mps[i][j] && !mps[i][j]->isBad();", "good[i][j] = mps[i][j] != nullptr;", F_MW, "SearchByBoW(KeyFrame, Frame), resident form: bad points take part")
M(2051, FH, "const size_t lim1 = pKF1->NLeft != -1 ?", "const size_t lim1 = pKF1->NLeft == -1 ?", F_MW, "SearchByBoW(KeyFrame, KeyFrame): camera 2's features of key frame 1 take part")
M(2052, FH, "lim2 = pKF2->NLeft != -1 ?", "lim2 = pKF2->NLeft == -1 ?", F_MW, "SearchByBoW(KeyFrame, KeyFrame): camera 2's features of key frame 2 take part")
M(2053, FH, "k1.present[i] = vpMapPoints1[i] && !vpMapPoints1[i]->isBad();", "k1.present[i] = vpMapPoints1[i] != nullptr;", F_MW, "SearchByBoW(KeyFrame, KeyFrame): bad points of key frame 1 take part")
M(2054, FH, "k2.present[i] = vpMapPoints2[i] && !vpMapPoints2[i]->isBad();", "k2.present[i] = vpMapPoints2[i] != nullptr;", F_MW, "SearchByBoW(KeyFrame, KeyFrame): bad points of key frame 2 take part")
M(2055, FH, "&k1.v, &k2.v, mfNNratio, 1, mbCheckOrientation, m12.data(), &nmatches));", "&k1.v, &k2.v, mfNNratio, 0, mbCheckOrientation, m12.data(), &nmatches));", F_MW,
  "SearchByBoW(KeyFrame, Frame), uploaded form: the key-frame pair's threshold (< TH_LOW)")
M(2056, FH, "&k1.v, &k2.v, mfNNratio, 0, mbCheckOrientation, m12.data(), &nmatches));", "&k1.v, &k2.v, mfNNratio, 1, mbCheckOrientation, m12.data(), &nmatches));", F_MW,
  "SearchByBoW(KeyFrame, KeyFrame): the frame form's threshold (<= TH_LOW)")
M(2057, FH, "k2.data(), nullptr, mfNNratio, 1, mbCheckOrientation, m12p.data(), counts.data());", "k2.data(), nullptr, mfNNratio, 0, mbCheckOrientation, m12p.data(), counts.data());", F_MW,
  "SearchByBoW(KeyFrame, Frame), resident form: the key-frame pair's threshold (< TH_LOW)")
M(2058, FH, "{ vnMatches12[i] = m12[i]; vbPrevMatched[i].x = prev[2 * i]; vbPrevMatched[i].y = prev[2 * i + 1]; }", "{ vnMatches12[i] = m12[i]; }", F_MW, "SearchForInitialization: vbPrevMatched not written back")
# SearchForTriangulation
M(2060, FH, "if (pKF1->N > 0 && !pKF1->mFeatVec.empty() && !pKF2->mFeatVec.empty()) {", "if (pKF1->N > 0 && !pKF1->mFeatVec.empty()) {", F_MW, "SearchForTriangulation: a second key frame without BoW takes the resident route", ROUTE)
M(2061, FH, "mp1[i] = pKF1->GetMapPoint(i) != nullptr;", "mp1[i] = 0;", F_MW, "SearchForTriangulation, resident form: features of key frame 1 with a point are searched")
M(2062, FH, "mp2[j][i] = pKF2->GetMapPoint(i) != nullptr;", "mp2[j][i] = 0;", F_MW, "SearchForTriangulation, resident form: features of key frame 2 with a point are candidates")
M(2064, FH, "kb.nleft1 = rig ? pKF1->NLeft : -1;", "kb.nleft1 = -1;", F_MW, "FillKB8Pair: key frame 1 of a rig pair judged as one camera")
M(2065, FH, "put(0, T1w * Tw2); put(1, T1w * Twr2);", "put(0, T1w * Tw2); put(1, T1w * Tw2);", F_MW, "FillKB8Pair: Tlr takes the left-left transform")
M(2067, FH, "if (pKF1->NLeft != -1) FillAllKeys(*pKF1, pKF1->NLeft, pKF1->N, k1);", "", F_MW, "SearchForTriangulation, fisheye, uploaded form: a rig key frame's keypoints from mvKeysUn")
M(2068, FH, "if (pKF->NLeft != -1) FillAllKeys(*pKF, pKF->NLeft, pKF->N, k);      // a rig", "     // a rig", F_MW + F_CACHE[4:6], "ResidentKeyFrames::Get: a rig key frame's keypoints from mvKeysUn")
# SearchBySim3
M(2070, FH, "if (!partner) continue;\n            paired[0][i] = 1;", "if (!partner) continue;", F_MW, "SearchBySim3: a point of key frame 1 that has a partner is searched")
M(2071, FH, "if (j >= 0 && j < n[1]) paired[1][j] = 1;", "if (j >= 0 && j < n[1]) paired[1][j] = 0;", F_MW, "SearchBySim3: the partner in key frame 2 is searched")
M(2072, FH, "if (pMP && !paired[side][i] && !pMP->isBad()) pts.take(i, pMP, false);", "if (pMP && !pMP->isBad()) pts.take(i, pMP, false);", F_MW, "SearchBySim3: paired points are searched")
M(2073, FH, "if (pMP && !paired[side][i] && !pMP->isBad()) pts.take(i, pMP, false);", "if (pMP && !paired[side][i]) pts.take(i, pMP, false);", F_MW, "SearchBySim3: bad points are searched")
M(2074, FH, "const Sim3T across[2] = {S12.inverse(), S12};", "const Sim3T across[2] = {S12, S12.inverse()};", F_MW, "SearchBySim3: the two directions' transforms swapped")
M(2075, FH, "spec.depth_test = 1; spec.dist_mode = 1; spec.distance_test = 1;", "spec.depth_test = 1; spec.dist_mode = 0; spec.distance_test = 1;", F_MW, "SearchBySim3: the range from the camera centre instead of |p_c|")
# Fuse, one key frame
M(2080, FH, "if (pMP && !pMP->isBad() && !pMP->IsInKeyFrame(pKF)) pts.take(i, pMP, true);", "if (pMP && !pMP->IsInKeyFrame(pKF)) pts.take(i, pMP, true);", F_FUSE, "Fuse, head: bad points are projected", TWICE)
M(2081, FH, "if (pMP && !pMP->isBad() && !pMP->IsInKeyFrame(pKF)) pts.take(i, pMP, true);", "if (pMP && !pMP->isBad()) pts.take(i, pMP, true);", F_FUSE, "Fuse, head: points of the key frame are projected", TWICE)
M(2082, FH, "if (!incoming || !ps.valid[i] || best[i] < 0 || incoming->isBad() || incoming->IsInKeyFrame(pKF)) continue;",
  "if (!incoming || !ps.valid[i] || best[i] < 0 || incoming->IsInKeyFrame(pKF)) continue;", F_FUSE, "Fuse, replay: a point that an earlier merge made bad is merged")
M(2083, FH, "if (!incoming || !ps.valid[i] || best[i] < 0 || incoming->isBad() || incoming->IsInKeyFrame(pKF)) continue;",
  "if (!incoming || !ps.valid[i] || best[i] < 0 || incoming->isBad()) continue;", F_FUSE, "Fuse, replay: a point that an earlier merge put into the key frame is merged")
M(2084, FH, "resident->Observations() > incoming->Observations() ? resident : incoming;\n                (keep == resident ? incoming : resident)->Replace(keep);\n            }\n            merged++;",
  "resident->Observations() >= incoming->Observations() ? resident : incoming;\n                (keep == resident ? incoming : resident)->Replace(keep);\n            }\n            merged++;", F_FUSE,
  "Fuse: with equal observations the resident point survives")
M(2085, FH, "if (resident && !resident->isBad()) {           // two points for one keypoint", "if (resident) {           // two points for one keypoint", F_FUSE, "Fuse: a bad resident point is merged with")
M(2086, FH, "if (best[i] >= 0) best[i] += pKF->NLeft;", "if (best[i] >= 0) best[i] += 0;", F_FUSE, "Fuse(bRight): the keypoint index without + NLeft")
M(2087, FH, "bRight ? Spec(pKF->GetRightPose(), pKF->mpCamera2,", "bRight ? Spec(pKF->GetPose(), pKF->mpCamera2,", F_FUSE, "Fuse(bRight): camera 1's pose")
M(2088, FH, "if (bRight) SpecCentre(spec, pKF->GetRightCameraCenter()); else", "if (!bRight) SpecCentre(spec, pKF->GetRightCameraCenter()); else", F_FUSE, "Fuse: the two cameras' centres swapped")
M(2089, FH, "spec.angle_test = 1; spec.bf = pKF->mbf;\n        pts.project(spec);", "spec.angle_test = 0; spec.bf = pKF->mbf;\n        pts.project(spec);", F_FUSE, "Fuse: the viewing-angle test switched off")
M(2090, FH, "ps.view(), th, 1, pKF->mvInvLevelSigma2.data(), best.data(), nullptr));", "ps.view(), th, 0, pKF->mvInvLevelSigma2.data(), best.data(), nullptr));", F_FUSE, "Fuse: the chi-square gate switched off")
M(2091, FH, "if (!there) { point->AddObservation(kf, slot); kf->AddMapPoint(point, slot); }", "if (!there) { kf->AddMapPoint(point, slot); }", F_FUSE, "Attach: AddObservation dropped")
M(2092, FH, "if (!there) { point->AddObservation(kf, slot); kf->AddMapPoint(point, slot); }", "if (!there) { point->AddObservation(kf, slot); }", F_FUSE, "Attach: AddMapPoint dropped")
M(2093, FH, "if (!pMP->isBad() && !inKeyFrame.count(pMP)) pts.take(i, pMP, true);", "if (!inKeyFrame.count(pMP)) pts.take(i, pMP, true);", F_FUSE, "Fuse(Sim3), head: bad points are projected")
M(2094, FH, "if (!pMP->isBad() && !inKeyFrame.count(pMP)) pts.take(i, pMP, true);", "if (!pMP->isBad()) pts.take(i, pMP, true);", F_FUSE, "Fuse(Sim3), head: points of the key frame are projected")
M(2095, FH, "if (!ps.valid[i] || best[i] < 0 || vpPoints[i]->isBad()) continue;", "if (!ps.valid[i] || best[i] < 0) continue;", F_FUSE, "Fuse(Sim3), replay: the isBad test removed",
  "equivalent: the head lets only points through that are not bad, ps.valid is 0 for every other, and nothing between head and replay of this overload changes a point's state "
  "(Attach adds an observation; Replace is the caller's, after the call)")
M(2096, FH, "if (resident && !resident->isBad()) vpReplacePoint[i] = resident;\n            merged++;", "if (resident) vpReplacePoint[i] = resident;\n            merged++;", F_FUSE, "Fuse(Sim3): a bad resident point is reported")
# (2093 and 2095 are the two places of ONE test: each alone is equivalent because the other still stands.  2097 takes both away)
M(2097, FH, "if (!pMP->isBad() && !inKeyFrame.count(pMP)) pts.take(i, pMP, true);", "if (!inKeyFrame.count(pMP)) pts.take(i, pMP, true);", F_FUSE, "Fuse(Sim3): isBad tested at neither place",
  more=[("if (!ps.valid[i] || best[i] < 0 || vpPoints[i]->isBad()) continue;", "if (!ps.valid[i] || best[i] < 0) continue;")])
# Fuse, many key frames
M(2100, FH, "return !p || p->isBad() || p->IsInKeyFrame(pKF); };", "return !p || p->IsInKeyFrame(pKF); };", F_FUSE, "Fuse, many: bad points are searched", TWICE)
M(2101, FH, "return !p || p->isBad() || p->IsInKeyFrame(pKF); };", "return !p || p->isBad(); };", F_FUSE, "Fuse, many: points of the key frame are searched", TWICE)
M(2102, FH, "if (pKF->NLeft != -1) continue;\n                OrbmProjection spec = Spec(pKF->GetPose(), pKF->mpCamera, *pKF, /*IsInImage*/ 1);",
  "OrbmProjection spec = Spec(pKF->GetPose(), pKF->mpCamera, *pKF, /*IsInImage*/ 1);", F_FUSE, "Fuse, many: a rig key frame takes the batched route")
M(2103, FH, "if (pKF->NLeft != -1) counts[k] += Fuse(pKF, vpMapPoints, true);", "", F_FUSE, "Fuse, many: a rig key frame's second pass dropped")
M(2104, FH, "if (pKF->NLeft != -1) counts[k] += Fuse(pKF, vpMapPoints, true);", "if (pKF->NLeft != -1) counts[k] += Fuse(pKF, vpMapPoints, th, true);", F_FUSE,
  "Fuse, many: a rig key frame's second pass searches camera 2 (the reference's call site passes `true` as th)")
M(2105, FH, "if (batched) job.NoteChangedDescriptors();", "", F_FUSE, "Fuse, many: no refresh behind a key frame that took the unbatched route")
M(2106, FH, "if (!incoming || best[i] < 0 || incoming->isBad() || incoming->IsInKeyFrame(pKF)) continue;", "if (!incoming || best[i] < 0 || incoming->IsInKeyFrame(pKF)) continue;", F_FUSE,
  "Fuse, many, replay: a point that an earlier merge made bad is merged")
M(2107, FH, "if (!incoming || best[i] < 0 || incoming->isBad() || incoming->IsInKeyFrame(pKF)) continue;", "if (!incoming || best[i] < 0 || incoming->isBad()) continue;", F_FUSE,
  "Fuse, many, replay: a point that an earlier merge put into the key frame is merged")
M(2108, FH, "resident->Observations() > incoming->Observations() ? resident : incoming;\n                    (keep == resident ? incoming : resident)->Replace(keep);\n                    job.NoteChangedDescriptorOf(keep);",
  "resident->Observations() >= incoming->Observations() ? resident : incoming;\n                    (keep == resident ? incoming : resident)->Replace(keep);\n                    job.NoteChangedDescriptorOf(keep);", F_FUSE,
  "Fuse, many: with equal observations the resident point survives")
M(2109, FH, "job.NoteChangedDescriptorOf(keep);       // (either", ";       // (either", F_FUSE, "Fuse, many: the survivor of a Replace is not searched again")
M(2110, FH, "job.Refresh(row, excluded);\n            const int* best = job.Best(row);", "const int* best = job.Best(row);", F_FUSE, "Fuse, many: no Refresh in front of a key frame's replay")
M(2111, FH, "if (resident && !resident->isBad()) {\n                    MapPointT* keep", "if (resident) {\n                    MapPointT* keep", F_FUSE, "Fuse, many: a bad resident point is merged with")
M(2112, FH, "return vpPoints[i]->isBad() || job.Holds(pKF, vpPoints[i]); };", "return job.Holds(pKF, vpPoints[i]); };", F_FUSE, "Fuse(Sim3), many: bad points are searched",
  "equivalent: the replay loop of this overload tests vpPoints[i]->isBad() again before anything is written, and a bad point's search result is read nowhere else")
M(2113, FH, "return vpPoints[i]->isBad() || job.Holds(pKF, vpPoints[i]); };", "return vpPoints[i]->isBad(); };", F_FUSE, "Fuse(Sim3), many: points of the key frame are searched",
  "equivalent: the replay loop reads pKF->GetMapPoints() at its own moment, which holds whatever Holds held, and skips those points")
M(2114, FH, "job.Refresh(row, excluded);\n                const int* best = job.Best(row);", "const int* best = job.Best(row);", F_FUSE, "Fuse(Sim3), many: no Refresh in front of a key frame's replay")
M(2115, FH, "if (best[i] < 0 || vpPoints[i]->isBad() || inKeyFrame.count(vpPoints[i])) continue;", "if (best[i] < 0 || inKeyFrame.count(vpPoints[i])) continue;", F_FUSE,
  "Fuse(Sim3), many, replay: a point that an earlier hook made bad is attached")
M(2116, FH, "if (best[i] < 0 || vpPoints[i]->isBad() || inKeyFrame.count(vpPoints[i])) continue;", "if (best[i] < 0 || vpPoints[i]->isBad()) continue;", F_FUSE,
  "Fuse(Sim3), many, replay: a point that an earlier hook put into the key frame is attached")
M(2117, FH, "if (resident && !resident->isBad()) vpReplacePoint[i] = resident;\n                    counts[k]++;", "if (resident) vpReplacePoint[i] = resident;\n                    counts[k]++;", F_FUSE,
  "Fuse(Sim3), many: a bad resident point is reported")
M(2118, FH, "if (batched) for (int i = 0; i < M; i++) if (vpReplacePoint[i] && !vpPoints[i]->isBad()) job.NoteChangedDescriptorOf(vpPoints[i]);", "", F_FUSE,
  "Fuse(Sim3), many: what the hook changed is not searched again")
M(2119, FH, "if (pKF->NLeft != -1) continue;\n                const SE3T pose = RigidPart<SE3T>(vScw[k]);", "const SE3T pose = RigidPart<SE3T>(vScw[k]);", F_FUSE, "Fuse(Sim3), many: a rig key frame takes the batched route")
# FuseBatch
M(2121, FH, "heldOf = nullptr;\n            OrbmWorldPointView view = {n,", "OrbmWorldPointView view = {n,", F_FUSE, "FuseBatch::Run: the held set of the last key frame stays valid after the exclusion loop")
M(2122, FH, "heldOf = nullptr;\n            for (int r = 0; r < rows; r++) for (int j = 0; j < n; j++) skip", "for (int r = 0; r < rows; r++) for (int j = 0; j < n; j++) skip", F_FUSE,
  "FuseBatch::Run: the held set is not forgotten in front of the exclusion loop")
# (2121 and 2122 are likewise a pair: either reset alone forgets the held set between two runs.  2123 takes both away)
M(2123, FH, "heldOf = nullptr;\n            OrbmWorldPointView view = {n,", "OrbmWorldPointView view = {n,", F_FUSE, "FuseBatch::Run: the held set is never forgotten",
  more=[("heldOf = nullptr;\n            for (int r = 0; r < rows; r++) for (int j = 0; j < n; j++) skip", "for (int r = 0; r < rows; r++) for (int j = 0; j < n; j++) skip")])
M(2124, FH, "{ memcpy(&desc[32 * (size_t)i], now, 32); stale.push_back(i); }", "{ stale.push_back(i); }", F_FUSE, "FuseBatch::NoteChangedDescriptor: the new descriptor is not kept")
M(2125, FH, "{ memcpy(&desc[32 * (size_t)i], now, 32); stale.push_back(i); }", "{ memcpy(&desc[32 * (size_t)i], now, 32); }", F_FUSE, "FuseBatch::NoteChangedDescriptor: the point is not marked stale")
M(2126, FH, "if (points[i] && !points[i]->isBad()) NoteChangedDescriptor(i); }", "if (points[i]) NoteChangedDescriptor(i); }", F_FUSE, "FuseBatch::NoteChangedDescriptors: bad points are compared too",
  "equivalent: a bad point is excluded by every later search and replay (`excluded`, the replay's own isBad), so whether its row is searched again changes nothing that is read")
M(2128, FH, "for (int j = 0; j < n; j++) row[subset[j]] = -1;", "", F_FUSE, "FuseBatch::Run: a point searched again keeps its old candidate when the new search finds none")
M(2129, FH, "for (auto it = range.first; it != range.second; ++it) NoteChangedDescriptor(it->second);", "if (range.first != range.second) NoteChangedDescriptor(range.first->second);", F_FUSE,
  "FuseBatch::NoteChangedDescriptorOf: only the first place of a point listed twice")
# ResidentKeyFrames
M(2140, FH, "return id == o.id && n == o.n && nodes == o.nodes && print == o.print; }", "return n == o.n && nodes == o.nodes && print == o.print; }", F_CACHE, "ResidentKeyFrames::Tag: mnId not compared")
M(2141, FH, "return id == o.id && n == o.n && nodes == o.nodes && print == o.print; }", "return id == o.id && nodes == o.nodes && print == o.print; }", F_CACHE, "ResidentKeyFrames::Tag: N not compared")
M(2142, FH, "return id == o.id && n == o.n && nodes == o.nodes && print == o.print; }", "return id == o.id && n == o.n && print == o.print; }", F_CACHE, "ResidentKeyFrames::Tag: the size of mFeatVec not compared")
M(2143, FH, "return id == o.id && n == o.n && nodes == o.nodes && print == o.print; }", "return id == o.id && n == o.n && nodes == o.nodes; }", F_CACHE, "ResidentKeyFrames::Tag: the fingerprint not compared")
M(2144, FH, "if (pKF->N > 0 && pKF->mFeatVec.empty()) { transient = r; return r; }", "", F_CACHE, "ResidentKeyFrames::Get: a key frame without BoW is cached")
M(2145, FH, "if (transient) { orbm_keyframe_destroy(transient); transient = nullptr; }\n            BowStore k;", "BowStore k;", F_CACHE, "ResidentKeyFrames::Get: the previous transient entry is not released (a leak)")
M(2146, FH, "if (device != Device()) { Clear(); device = Device(); }\n            const Tag tag = {(long long)pKF->mnId, (long long)pKF->N, (long long)pKF->mFeatVec.size(), Fingerprint(pKF)};\n            auto it = m.find(pKF);\n            if (it != m.end()) {\n                if",
  "if (device != Device()) { device = Device(); }\n            const Tag tag = {(long long)pKF->mnId, (long long)pKF->N, (long long)pKF->mFeatVec.size(), Fingerprint(pKF)};\n            auto it = m.find(pKF);\n            if (it != m.end()) {\n                if",
  F_CACHE, "ResidentKeyFrames::Get: the cache survives a change of device")
M(2148, FH, "{ it->second.stamp = ++clock; return it->second.dev; }", "{ return it->second.dev; }", F_CACHE, "ResidentKeyFrames::Get: a hit does not renew the entry's age")
M(2149, FH, "if (capacity == 0 || m.size() <= capacity) return;", "if (capacity == 0 || m.size() < capacity) return;", F_CACHE, "ResidentKeyFrames::Trim: a cache of exactly `capacity` entries is trimmed")
M(2150, FH, "m.size() - capacity + capacity / 8;", "m.size() - capacity + capacity / 9;", F_CACHE, "ResidentKeyFrames::Trim: capacity / 9 below the bound")
M(2151, FH, "byAge.begin() + (drop < byAge.size() ? drop : byAge.size() - 1), byAge.end());", "byAge.begin() + (drop < byAge.size() ? drop - 1 : byAge.size() - 1), byAge.end());", F_CACHE,
  "ResidentKeyFrames::Trim: nth_element at drop - 1",
  "equivalent: drop >= 1 here; with the nth element at index drop - 1 the entries in front of it are not younger than it, so [0, drop) is the same set of the `drop` oldest entries (stamps are unique)")
M(2152, FH, "std::nth_element(byAge.begin(), byAge.begin() + (drop < byAge.size() ? drop : byAge.size() - 1), byAge.end());", "", F_CACHE, "ResidentKeyFrames::Trim: entries dropped in address order, not by age")
M(2154, FH, "if (it->second.dev != dev) orbm_keyframe_destroy(it->second.dev);", "", F_CACHE, "ResidentKeyFrames::Adopt: the entry it replaces is not destroyed (a leak)")
M(2156, FH, "SetCapacity(n ? n : 1); }", "SetCapacity(n); }", F_CACHE, "SetImplicitCapacity(0) sets 0, which the next ImplicitCache() turns into 256")
M(2157, FH, "if (c.Capacity() == 0) c.SetCapacity((size_t)kImplicitCacheEntries);", "", F_CACHE, "ImplicitCache: unbounded")
M(2158, FH, "if (capacity == 0 || m.size() <= capacity) return;", "if (m.size() <= capacity) return;", F_CACHE, "ResidentKeyFrames::Trim: capacity 0 empties the cache")
# occupancy
M(2165, FH, "F.mvpMapPoints[first + i]->Observations() > 0;", "F.mvpMapPoints[first + i]->Observations() >= 0;", F_MW, "FillOccupancy: a point without observations occupies under OccupiedWithObservations")
M(2166, FH, "FillOccupancy(F, NL, NR, occ, s.r.occ);", "FillOccupancy(F, 0, NR, occ, s.r.occ);", F_MW, "FillRig: camera 2's occupancy read at camera 1's slots")
# the stereo free functions
F_TAIL = [FG, MOCK]
M(2170, FH, "F.mvuRight = std::vector<float>(F.Nleft, -1);", "F.mvuRight = std::vector<float>(F.Nleft, 0);", F_TAIL, "ComputeStereoFishEyeMatches: mvuRight reset to 0")
M(2171, FH, "F.mnCloseMPs = 0;", "", F_TAIL, "ComputeStereoFishEyeMatches: mnCloseMPs not reset")
M(2172, FH, "if (l2r[i] >= 0) F.mvStereo3Dpoints[i] =", "if (l2r[i] > 0) F.mvStereo3Dpoints[i] =", F_TAIL, "ComputeStereoFishEyeMatches: a match with right keypoint 0 gets no 3-D point")
M(2173, FH, "F.mvRightToLeftMatch.assign(r2l.begin(), r2l.begin() + F.Nright);", "F.mvRightToLeftMatch.assign(l2r.begin(), l2r.begin() + F.Nright);", F_TAIL, "ComputeStereoFishEyeMatches: mvRightToLeftMatch from the left table")

FK = "include/orb_slam3_amd/KeyFrameDatabase.h"
M(2200, FK, "e.n++;", "e.n = 1;", F_KFDB, "add: a second add of the same key frame is not counted")
M(2201, FK, "if (--it->second.n == 0) mAdds.erase(it);", "mAdds.erase(it);", F_KFDB, "erase: the first erase forgets a key frame that was added twice")
M(2202, FK, "if (--it->second.n == 0) mAdds.erase(it);", "if (--it->second.n <= 1) mAdds.erase(it);", F_KFDB, "erase: a key frame with one surviving add is forgotten")
M(2203, FK, "if (it->second.mapOf(it->first) == (const void*)pMap)", "if (it->second.mapOf(it->first) != (const void*)pMap)", F_KFDB, "clearMap: the other maps' key frames are erased")
M(2204, FK, "if (pKFi->mnRelocQuery != F->mnId) { pKFi->mnRelocWords = 0;", "if (pKFi->mnRelocQuery != F->mnId) {", F_KFDB, "reloc: the word counter is not reset")
M(2205, FK, "pKFi->mnRelocQuery = F->mnId; lKFsSharingWords.push_back(pKFi); }\n            else repeat = true;", "pKFi->mnRelocQuery = F->mnId; lKFsSharingWords.push_back(pKFi); }", F_KFDB, "reloc: a repeat query id is not noticed")
M(2206, FK, "if (k->mnRelocWords > maxCommonWords) maxCommonWords = k->mnRelocWords;\n        int minCommonWords = maxCommonWords * 0.8f;", "if (k->mnRelocWords > maxCommonWords) maxCommonWords = k->mnRelocWords;\n        int minCommonWords = maxCommonWords * 0.7f;", F_KFDB, "reloc: 0.7f of the most common words")
M(2207, FK, "if (pKFi->mnRelocWords > minCommonWords) {", "if (pKFi->mnRelocWords >= minCommonWords) {", F_KFDB, "reloc: exactly minCommonWords is enough")
M(2208, FK, "if (pKF2->mnRelocQuery != F->mnId) continue;", "", F_KFDB, "reloc: a neighbour that this query did not stamp adds its old score")
M(2209, FK, "accScore += pKF2->mRelocScore;", "", F_KFDB, "reloc: the neighbours' scores are not accumulated")
M(2210, FK, "if (pKF2->mRelocScore > bestScore) { pBestKF = pKF2;", "if (pKF2->mRelocScore >= bestScore) { pBestKF = pKF2;", F_KFDB, "reloc: a neighbour with the same score becomes the group's key frame")
M(2211, FK, "{ pBestKF = pKF2; bestScore = pKF2->mRelocScore; }", "{ pBestKF = pKF2; }", F_KFDB, "reloc: the best score of the group is not raised")
M(2212, FK, "if (accScore > bestAccScore) bestAccScore = accScore;\n        }\n        float minScoreToRetain = 0.75f * bestAccScore;", "if (accScore < bestAccScore) bestAccScore = accScore;\n        }\n        float minScoreToRetain = 0.75f * bestAccScore;", F_KFDB,
  "reloc: the best accumulated score is never raised")
M(2213, FK, "float minScoreToRetain = 0.75f * bestAccScore;", "float minScoreToRetain = 0.8f * bestAccScore;", F_KFDB, "reloc: 0.8f of the best accumulated score")
M(2214, FK, "if (si > minScoreToRetain) {", "if (si >= minScoreToRetain) {", F_KFDB, "reloc: exactly 0.75f of the best accumulated score is enough")
M(2215, FK, "if (pKFi->GetMap() != pMap) continue;", "", F_KFDB, "reloc: candidates of other maps are returned")
M(2216, FK, "if (!spAlreadyAddedKF.count(pKFi)) { vpRelocCandidates.push_back(pKFi);", "{ vpRelocCandidates.push_back(pKFi);", F_KFDB, "reloc: a key frame that leads two groups is returned twice")
M(2217, FK, "if (repeat) { Query(bow, excluded, all, 1); src = &all; }", "", F_KFDB, "Scores: no rescoring after a repeat query id")
M(2220, FK, "if (pKFi->mnPlaceRecognitionQuery != pKF->mnId) { pKFi->mnPlaceRecognitionWords = 0;", "if (pKFi->mnPlaceRecognitionQuery != pKF->mnId) {", F_KFDB, "nbest: the word counter is not reset")
M(2221, FK, "if (c->mnPlaceRecognitionQuery != pKF->mnId) c->mnPlaceRecognitionWords = 1;", "if (c->mnPlaceRecognitionQuery != pKF->mnId) c->mnPlaceRecognitionWords = shared;", F_KFDB,
  "nbest: a connected key frame's counter holds its shared words, not the reference's single 1")
M(2222, FK, "else c->mnPlaceRecognitionWords += shared;", "else c->mnPlaceRecognitionWords += 1;", F_KFDB, "nbest: a connected key frame stamped earlier counts one word")
M(2223, FK, "SharedWords(pKF->mBowVec, c->mBowVec) * it->second.n;", "SharedWords(pKF->mBowVec, c->mBowVec);", F_KFDB, "nbest: a connected key frame that was added twice counts its words once")
M(2224, FK, "if (shared == 0) continue;", "", F_KFDB, "nbest: a connected key frame without shared words gets the 1")
M(2225, FK, "if (k->mnPlaceRecognitionWords > maxCommonWords) maxCommonWords = k->mnPlaceRecognitionWords;\n        int minCommonWords = maxCommonWords * 0.8f;",
  "if (k->mnPlaceRecognitionWords > maxCommonWords) maxCommonWords = k->mnPlaceRecognitionWords;\n        int minCommonWords = maxCommonWords * 0.7f;", F_KFDB, "nbest: 0.7f of the most common words")
M(2226, FK, "if (pKFi->mnPlaceRecognitionWords > minCommonWords) {", "if (pKFi->mnPlaceRecognitionWords >= minCommonWords) {", F_KFDB, "nbest: exactly minCommonWords is enough")
M(2227, FK, "if (pKF2->mnPlaceRecognitionQuery != pKF->mnId) continue;", "", F_KFDB, "nbest: a neighbour that this query did not stamp adds its old score")
M(2228, FK, "if (pKF2->mPlaceRecognitionScore > bestScore) { pBestKF = pKF2;", "if (pKF2->mPlaceRecognitionScore >= bestScore) { pBestKF = pKF2;", F_KFDB, "nbest: a neighbour with the same score becomes the group's key frame")
M(2230, FK, "lAccScoreAndMatch.sort([]", "lAccScoreAndMatch.reverse(); lAccScoreAndMatch.sort([]", F_KFDB, "nbest: equal accumulated scores in the reverse order of the list")
M(2231, FK, "while (i < lAccScoreAndMatch.size() && ((int)vpLoopCand.size() < nNumCandidates || (int)vpMergeCand.size() < nNumCandidates)) {",
  "while (i < lAccScoreAndMatch.size() && ((int)vpLoopCand.size() < nNumCandidates && (int)vpMergeCand.size() < nNumCandidates)) {", F_KFDB, "nbest: the walk ends when ONE of the lists is full")
M(2232, FK, "if (pKF->GetMap() == pKFi->GetMap() && (int)vpLoopCand.size() < nNumCandidates) vpLoopCand.push_back(pKFi);", "if (pKF->GetMap() == pKFi->GetMap() && (int)vpLoopCand.size() <= nNumCandidates) vpLoopCand.push_back(pKFi);", F_KFDB,
  "nbest: one loop candidate more than asked")
M(2233, FK, "(int)vpMergeCand.size() < nNumCandidates && !pKFi->GetMap()->IsBad()) vpMergeCand.push_back(pKFi);", "(int)vpMergeCand.size() <= nNumCandidates && !pKFi->GetMap()->IsBad()) vpMergeCand.push_back(pKFi);", F_KFDB,
  "nbest: one merge candidate more than asked")
M(2234, FK, " && !pKFi->GetMap()->IsBad()) vpMergeCand.push_back(pKFi);", ") vpMergeCand.push_back(pKFi);", F_KFDB, "nbest: a key frame of a bad map is a merge candidate")
M(2235, FK, "else if (pKF->GetMap() != pKFi->GetMap() && (int)vpMergeCand.size()", "else if ((int)vpMergeCand.size()", F_KFDB, "nbest: a key frame of the query's map beyond the loop list's end becomes a merge candidate")
M(2236, FK, "if (!spAlreadyAddedKF.count(pKFi)) {\n                if (pKF->GetMap()", "{\n                if (pKF->GetMap()", F_KFDB, "nbest: a key frame that leads two groups is listed twice")
M(2237, FK, "for (KeyFrameT* k : spConnectedKF) excluded.push_back(Key(k));", "", F_KFDB, "nbest: connected key frames are not excluded from the query")
M(2238, FK, "pKFi->mnPlaceRecognitionQuery = pKF->mnId; lKFsSharingWords.push_back(pKFi); }\n            else repeat = true;", "pKFi->mnPlaceRecognitionQuery = pKF->mnId; lKFsSharingWords.push_back(pKFi); }", F_KFDB,
  "nbest: a repeat query id is not noticed")

FX = "include/orb_slam3_amd/ORBextractor.h"
M(2260, FX, "attempt < 2 && rc == ORBX_E_CAPACITY; attempt++)", "attempt < 1 && rc == ORBX_E_CAPACITY; attempt++)", F_EXTRACT, "ORBextractor: no second attempt after ORBX_E_CAPACITY")
M(2261, FX, "const int c = attempt == 0 ? cap : std::max(orbx_max_keypoints(mpHandle), n);", "const int c = cap;", F_EXTRACT, "ORBextractor: the second attempt with the first one's capacity")
M(2263, FX, "b ? EDGE : 0, RING)", "EDGE, RING)", F_EXTRACT, "SetExportPyramid(false) leaves the device export on")
M(2264, FX, "mbExportPyramid = b;", "", F_EXTRACT, "SetExportPyramid: the flag is not kept")
M(2265, FX, "if(_image.empty())\n            return -1;", "if(_image.empty())\n            return 0;", F_EXTRACT, "ORBextractor: an empty image returns 0")

FV = "include/orb_slam3_amd/ORBVocabulary.h"
M(2280, FV, "v.clear(); fv.clear();", "", F_VOC, "ORBVocabularyAmd::transform: the output vectors are not cleared")
M(2281, FV, "if (v_) { orbv_destroy(v_); v_ = nullptr; }\n        return", "return", F_VOC, "ORBVocabularyAmd::loadFromTextFile: a second load leaks the first vocabulary")

# notes of the facade block, written after its pass (profiles/emu_mutants_facade/README.md): kept in one place because most of them argue from the same few facts
_SAME_RIG = ("no reference answer where it differs: the condition is reached with a frame and a key frame of different kinds (a rig frame against a one-camera key frame, or the "
             "other way round), which the reference never pairs - Tracking builds frames and key frames from one System, all with or all without mpCamera2 (src/Tracking.cc:1132, "
             "src/KeyFrame.cc:56-77 copies the frame's cameras) - and for two of one kind the other clauses of the line decide alone")
_FACADE_NOTES = {
    2019: "no accepted input reaches the difference: camera 2's projection of a point that camera 1 accepted is rejected by the added test only when the point lies BEHIND camera 2 "
          "(1 / z < 0 after GetRelativePoseTrl()); the Kannala-Brandt model puts such a point at a radius of more than fx * pi / 2 from the principal point (theta > pi / 2, "
          "csrc/kb8_model.h), outside every key point of an image that is narrower than that on each side of it - and the reference only builds rigs of Kannala-Brandt cameras "
          "(src/Tracking.cc:1132), whose frames lie inside that radius (752 x 480 at fx = 190 .. 435 in every rig of the suite)",
    2020: "equivalent but for z = -0.0f: depth_test 1 rejects z < 0, depth_test 2 rejects 1 / z < 0 (csrc/k_search.hip project_point), the same set for every other float "
          "(1 / z of a negative denormal is -inf); at -0 the reference's own u = fx * x * (1 / z) is an infinity or NaN that it converts to cell indices (src/Frame.cc:720-745): "
          "there is no defined answer to be compared with",
    2046: _SAME_RIG, 2047: _SAME_RIG,
    2055: "unreachable: the one-camera uploaded form is entered only when the first line of the method did not take the resident route, i.e. with pKF->mFeatVec empty (a rig goes to the "
          "fisheye call below it); without vocabulary nodes on the key frame's side there is no node pair, nothing is compared and the threshold is never read",
    2067: "unreachable: SearchForTriangulationFisheye is entered only when the resident route was not taken, i.e. when N == 0 or one of the two mFeatVec is empty; without common "
          "vocabulary nodes no pair of features is compared and the key points are never read",
    2093: "one of a redundant pair: the replay loop of this overload tests vpPoints[i]->isBad() again before anything is written; a bad point that the head lets through is "
          "projected, searched and skipped there.  2095 is the other place; the pair as a whole is mutant 2097, which takes both tests away",
    2121: "one of a redundant pair: Holds is called from the exclusion loop of Run alone, and 2122's reset in front of the loop still forgets the held set between two runs "
          "(the hooks that change a key frame's points run between them).  The pair as a whole is mutant 2123, which takes both resets away",
    2122: "the other of the redundant pair of 2121: the reset behind the loop has already forgotten the set when the next Run begins.  Both together: 2123",
    2123: "equivalent in the result: between two runs the set a key frame holds only grows by points that are not bad (a point leaves a key frame only by being replaced, and "
          "is bad from then on - excluded by the clause in front of Holds), and a point that has entered since is searched in vain: the replay loop reads "
          "pKF->GetMapPoints() at its own moment and skips it (the argument of 2113, where Holds goes altogether)",
    2260: "unreachable: ORBX_E_CAPACITY of orbx_extract needs n > cap, and the first attempt's cap is orbx_max_keypoints() >= the sum over the levels of quota + 3 - before the "
          "geometry is known that very sum (csrc/orbx_api.cpp:653-657), afterwards kp_total_cap, which is larger (:283) -, while a level never returns more than quota + 3 key points "
          "(`a full pass never overshoots the quota, a final-round split adds at most 3`, :282); the second attempt exists for a library whose bound changes, not for this one",
    2261: "unreachable, as 2260: the second attempt is never made",
    2263: "equivalent in every output: SetExportPyramid(false) clears mbExportPyramid, so operator() never asks for the exported levels; whether the device goes on writing them "
          "into its export slot is invisible to the caller (tests/cpp/pyramid_export_facade_test.cpp requires mvImagePyramid to keep its views) - it costs the time the switch "
          "was added to save, which tools/bench_dropin_frame.py measures",
}
for _m in MUTANTS:
    if _m["id"] in _FACADE_NOTES:
        assert not _m["note"], _m["id"]
        _m["note"] = _FACADE_NOTES[_m["id"]]


# ---- the state-carrying code: the resident map, the resident key frames, the key frame database (ids from 3000) ----------------------------------------------
# Kernels of k_search.hip / k_vocab.hip that no earlier block touches, the resident-map and batch host code of orbm_search.cpp, and the database of orbv_api.cpp.
# Not in the list, because the mutant could store outside an array once a test reaches it (the list's safety rule):
#   k_map_scan's loop bound and its carry `run += __shfl(incl, 63)` (the two pilot mutants), the chunk counts of k_map_compact and every rank moved UP: M_out shrinks or an
#   offset grows, the host lays the set out for the smaller M, and the scatter of k_map_compact then stores behind it.  The carry is mutated where it only moves stores DOWN
#   (3010); M_out itself is compared by tests/test_map_scan_tiles.py.
#   block_ballot_rank counting the lane's own wave (feat[at] behind the frame's row), `head` of k_map_set_flags without its imin (bytes behind the last frame's flags),
#   the remap of db_compact (a stale record index reads behind `mult`), every `slot >= m->slots` / `row >= m->kf_rows` / `feat >= kf_n` refusal (used as an index).
F = "k_search.hip"
M_BUILD = ["test_map_state_gates.py", "test_map_scan_tiles.py", "test_state_gaps.py", "test_local_map_build.py::test_list_emulated", "test_local_map_build.py::test_fields_emulated",
           "test_local_map_build.py::test_refusals_and_lifetime_emulated", "test_local_map_build.py::test_fuzz_emulated"]
M_SKIP = ["test_map_set_duplicates.py", "test_fuse_map.py", "test_sim3_map.py", "test_fuse_pairs.py"]
M_FLAGS = ["test_map_set_flags.py", "test_local_map_search.py", "test_sim3_map.py"]
M_ROWS = ["test_map_rows_resident.py", "test_map_rows_bow.py", "test_map_rows_projection.py"]
M_STEREO = ["test_stereo_points.py", "test_state_gaps.py"]
M_KF = ["test_keyframe_extracted.py", "test_resident_keyframes.py"]
KFDB = ["test_kfdb_state.py", "test_emu_kfdb.py", "test_kfdb_gates.py", "test_kfdb_reference.py"]
EARLY = ("equivalent in every output: the clear only comes one call earlier - a cleared table and a base of 0 give what a fresh map gives, which is what "
         "tests/test_map_scan_tiles.py and tests/test_map_set_duplicates.py require of every call on both sides of the limit")
# k_map_scatter, k_map_seen, map_visit, k_map_stamp
M(3000, F, "const uint8_t st = (uint8_t)(kMapPresent | (bad[r] ? kMapBad : 0));\n    if (!desc) {", "const uint8_t st = (uint8_t)(kMapPresent);\n    if (!desc) {", M_BUILD, "map scatter: the bad flag of the staged record ignored")
M(3001, F, "if (i < seen_start[b + 1]) seen_stamp[", "if (i + 1 < seen_start[b + 1]) seen_stamp[", M_BUILD, "map seen: the last slot of a frame's seen list is not marked")
M(3002, F, "seen_slots[i]] = mark;", "seen_slots[i]] = mark - 1u;", M_BUILD, "map seen: marked with the previous call's epoch")
M(3003, F, "return slot >= 0 && state[slot] == kMapPresent ? slot : -1;", "return slot > 0 && state[slot] == kMapPresent ? slot : -1;", M_BUILD, "map_visit: slot 0 is never visited")
M(3004, F, "if (slot >= 0) atomicMax(&stamp[(size_t)G.set * nslots + slot], top - (unsigned)(G.pos0 + i));", "if (slot >= 0) atomicMax(&stamp[(size_t)G.set * nslots + slot], top - (unsigned)i);", M_BUILD,
  "map stamp: the position inside the row offered instead of the position in the walk")
# k_map_compact, k_map_scan, k_map_gather
M(3006, F, "const int slot = i < G.n ? map_visit(G, i, kf_slots, row_cap, state) : -1;\n    const bool keep", "const int slot = i + 1 < G.n ? map_visit(G, i, kf_slots, row_cap, state) : -1;\n    const bool keep", M_BUILD,
  "map compact: the last entry of every visited row passed over")
M(3007, F, "const bool keep = slot >= 0 && stamp[(size_t)G.set * nslots + slot] == top - (unsigned)(G.pos0 + i);", "const bool keep = slot >= 0;", M_BUILD, "map compact: repeats are kept")
M(3008, F, "for (int w = 0; w < wave; w++) at += wave_cnt[w];\n    sets[G.set].slots[at] = slot;", "for (int w = 0; w < wave - 1; w++) at += wave_cnt[w];\n    sets[G.set].slots[at] = slot;", M_BUILD,
  "map compact: the rank inside a chunk forgets the wave in front")
M(3010, F, "if (i < c1) chunk_off[i] = run + incl - v;", "if (i < c1) chunk_off[i] = incl - v;", M_BUILD, "map scan: the offsets of a later tile forget the tiles in front")
M(3012, F, "(uint8_t)(seen_stamp[(size_t)R.set * nslots + slot] > base)", "(uint8_t)(seen_stamp[(size_t)R.set * nslots + slot] >= base)", M_BUILD, "map gather: a mark of the previous call reads as seen")
M(3013, F, "> base) : (uint8_t)0;", "> base) : (uint8_t)1;", M_BUILD + M_FLAGS[1:2], "map gather: the points of a selected set read as seen")
# k_map_rows_gather, k_map_row_flags
M(3014, F, "if (slot >= 0) {\n        const uint8_t st = S.state[slot];\n        ok =", "if (slot > 0) {\n        const uint8_t st = S.state[slot];\n        ok =", M_ROWS + ["test_state_gaps.py"], "rows gather: slot 0 holds no point")
M(3015, F, "flags[(size_t)R.off + i] = (uint8_t)(slot >= 0 && ", "flags[(size_t)R.off + i] = (uint8_t)(slot > 0 && ", M_ROWS + ["test_state_gaps.py"], "row flags: slot 0 holds no point")
# k_map_set_flags, k_assigned_slots
M(3016, F, "if (k < 4 ? k < head : o < M) { db[o] = src[o]; dobs[o] = 1; }", "if (k < 4 ? k + 1 < head : o < M) { db[o] = src[o]; dobs[o] = 1; }", M_FLAGS, "set flags: the last head byte is not copied")
M(3017, F, "if (k < 4 ? k < head : o < M) { db[o] = src[o]; dobs[o] = 1; }", "if (k < 4 ? k < head : o + 1 < M) { db[o] = src[o]; dobs[o] = 1; }", M_FLAGS, "set flags: the last tail byte is not copied")
M(3019, F, "if (k < 4 ? k < head : o < M) { db[o] = src[o]; dobs[o] = 1; }", "if (k < 4 ? k < head : o < M) { db[o] = src[o]; dobs[o] = 0; }", M_FLAGS, "set flags: the ragged ends have no observations")
M(3020, F, "*(uint32_t*)(dobs + o) = 0x01010101u;", "*(uint32_t*)(dobs + o) = 0x00010101u;", M_FLAGS, "set flags: every fourth point of the dword part has no observations")
M(3021, F, "db[o + 2] = src[o + 2]; db[o + 3] = src[o + 3]; }", "db[o + 2] = src[o + 2]; db[o + 3] = src[o + 2]; }", M_FLAGS, "set flags: the byte form copies a neighbour's flag")
M(3022, F, "if (agree) *(uint32_t*)(db + o) = *(const uint32_t*)(src + o);", "if (agree) *(uint32_t*)(db + o) = *(const uint32_t*)(src + o) & 0x00FFFFFFu;", M_FLAGS, "set flags: the dword form drops a flag")
M(3023, F, "out[o] = a < 0 ? a : (a < R.M ? R.slots[a] : -1);", "out[o] = a < 0 ? -1 : (a < R.M ? R.slots[a] : -1);", M_FLAGS, "assigned slots: every negative entry becomes -1",
  note="unreachable: the kernel has three callers - local_points_batch and local_points_rig_batch on a map's sets, and sim3_batch_run - and the accept kernels in front of it are the "
       "MapPoints forms local_accept_body<false> / rig_accept_body<false> and k_sim3_accept, which write an index or -1; the -2 of the rotation check is written under "
       "`LASTFRAME && check_ori` alone (k_search.hip, both bodies), and the last-frame batches return positions of the last frame's rows, which are never translated")
M(3024, F, "out[o] = a < 0 ? a : (a < R.M ? R.slots[a] : -1);", "out[o] = a <= 0 ? a : (a < R.M ? R.slots[a] : -1);", M_FLAGS, "assigned slots: the set's point 0 is not translated")
# k_map_skip_listed, k_map_skip_dups, k_fuse_kf_slots, k_map_edit_rows
M(3026, F, "if (slot < 0) return;\n    const unsigned t = table[slot], p = top - t;", "if (slot <= 0) return;\n    const unsigned t = table[slot], p = top - t;", M_SKIP, "skip listed: slot 0 in a list excludes nothing")
M(3027, F, "if (t > base && p < (unsigned)M) skip", "if (t > base && p + 1 < (unsigned)M) skip", M_SKIP, "skip listed: the set's last position is never excluded by a list")
M(3028, F, "if (first >= (unsigned)i) return; ", "if (first >= (unsigned)i || first == 0u) return; ", M_SKIP, "skip dups: a repeat of the slot at position 0 does not take its flag")
M(3029, F, "if (first >= (unsigned)i) return; ", "if (first > (unsigned)i) return; ", M_SKIP, "skip dups: a first position copies its own flag",
  note="equivalent: first == i reads skip[o + i] and stores 1 into the same byte only where it is 1 already")
M(3030, F, "if (b >= 0) {\n        const MapSkipRec R = recs[blockIdx.y];", "if (b > 0) {\n        const MapSkipRec R = recs[blockIdx.y];", M_SKIP, "fuse kf slots: a match with feature 0 reads as an empty entry")
M(3031, F, "if (j < n) kf_slots[(size_t)row[j] * (size_t)row_cap + (size_t)feat[j]] = slot[j];", "if (j + 1 < n) kf_slots[(size_t)row[j] * (size_t)row_cap + (size_t)feat[j]] = slot[j];", ["test_state_gaps.py"] + M_SKIP[1:2], "edit rows: the last edit of a call is dropped")
# k_map_stereo_select, k_map_stereo_write
M(3033, F, "const bool cand = d > 0.0f; ", "const bool cand = d >= 0.0f; ", M_STEREO, "stereo points: depth 0 is a candidate")
M(3034, F, "> P.th_depth && j + 1 > P.max_points) {", ">= P.th_depth && j + 1 > P.max_points) {", M_STEREO, "stereo points: depth == mThDepth counts as far")
M(3035, F, "> P.th_depth && j + 1 > P.max_points) {", "> P.th_depth && j + 1 >= P.max_points) {", M_STEREO, "stereo points: the stop rule fires at nPoints == max_points")
M(3036, F, "{ stop = (unsigned)(j + 1); break; }", "{ stop = (unsigned)j; break; }", M_STEREO, "stereo points: the walk ends in front of the first far entry")
M(3037, F, "const bool create = j < processed && !(keeps && keeps[f]);", "const bool create = j < processed;", M_STEREO, "stereo points: a feature that keeps its point gets a new one")
M(3040, F, "if (P.mode == 0) {\n        n0 =", "if (P.mode != 0) {\n        n0 =", M_STEREO, "stereo points: the normal's pass through UpdateNormalAndDepth belongs to the other mode")
M(3041, F, "if (R.row >= 0) kf_slots[(size_t)R.row * (size_t)row_cap + (size_t)i] = (int)slot; }", "if (R.row > 0) kf_slots[(size_t)R.row * (size_t)row_cap + (size_t)i] = (int)slot; }", M_STEREO, "stereo points: row 0 is not written")
# k_keyframe_counts
M(3042, F, "const int N = imin(*R.n_l, R.cap) + (R.kps_r ? imin(*R.n_r, R.cap) : 0);", "const int N = imin(*R.n_l, R.cap);", M_KF, "key frame counts: camera 2's features are not counted")
# k_sim3_candidates, k_sim3_accept
M(3050, F, "if (S.F.N > 0 && !(skip && skip[o]))", "if (S.F.N > 0)", SIM3[:2] + M_SKIP[:1], "Sim3 candidates: the skip mask ignored")
M(3051, F, "[occ](int idx) { return occ && occ[idx]; }", "[occ](int idx) { return false; }", SIM3[:2], "Sim3 candidates: keypoints occupied on entry are candidates",
  note="equivalent: k_sim3_candidates only proposes; k_sim3_accept starts its bitmap from the same occupancy on entry (s_occ from occ0) and walks the window again, against that "
       "bitmap, for every choice whose keypoint is taken in it (`if (pending && bit_of(s_occ, c))`), so a choice that fell on an occupied keypoint is replaced by the choice "
       "the unmutated kernel makes; it costs the second walk the candidates kernel exists to save")
M(3052, F, "const bool dirty = pending && s_claim[slot] < (unsigned)lane;", "const bool dirty = false;", SIM3[:2], "Sim3 accept: two points of one round take one keypoint")
M(3053, F, "if (i >= N || (occ0 && occ0[i]) || !bit_of(s_occ, i)) assigned[i] = -1;", "if (i >= N || !bit_of(s_occ, i)) assigned[i] = -1;", SIM3[:2], "Sim3 accept: a keypoint occupied on entry keeps what the array held")
# grid_build_body, k_lastframe_queries_rig, wave_find_node, k_bow_dists
M(3060, F, "if (!(px < 0 || px >= kGridCols || py < 0 || py >= kGridRows)) { myc[k] = px * kGridRows + py;", "if (!(px <= 0 || px >= kGridCols || py < 0 || py >= kGridRows)) { myc[k] = px * kGridRows + py;",
  ["test_state_gaps.py"] + FUSE[:2] + SIM3[:2] + M_KF, "key-frame grid: the first column of cells holds nothing")
M(3061, F, "while (j >= 0 && cell_items[st + j] > v)", "while (j >= 0 && cell_items[st + j] < v)", FUSE[:2] + SIM3[:2] + M_KF, "key-frame grid: a cell's items in descending index order")
M(3062, F, "if (after == 0) s_hist[c] = cur + before + 1;", "if (after == 0) s_hist[c] = cur + before;", FUSE[:2] + SIM3[:2] + M_KF + ["test_emu_search.py"], "key-frame grid, crowded cells: the cursor forgets the chunk's last item")
M(3065, F, "q.x = u; q.y = v; q.r = A.r; q.min_level = A.min_level; q.max_level = A.max_level; q.active = 1;", "q.x = u; q.y = v; q.r = A.r; q.min_level = A.min_level; q.max_level = -1; q.active = 1;",
  RIG[:1] + M_ROWS[2:], "last-frame rig queries: camera 2's window has no upper level")
M(3066, F, "const unsigned long long le = __ballot(pos < lo + len && ids[pos] <= id);", "const unsigned long long le = __ballot(pos < lo + len && ids[pos] < id);", ["test_state_gaps.py"] + BOW, "wave_find_node: a probe that hits the id does not count")
M(3067, F, "int d = -1;\n        if (eligible2[idx2]) {", "int d = -1;\n        if (!eligible2[idx2]) {", BOW, "bow dists: the eligibility flag negated")

# ---- k_match.hip: how k_distinctive_resident is fed ----
F = "k_match.hip"
M(3070, F, "const int r = first + k;\n    distinctive_point<kLds>", "const int r = k;\n    distinctive_point<kLds>", DISTINCTIVE, "distinctive (resident): the second form's launch starts at record 0 again")

# ---- k_vocab.hip ----
F = "k_vocab.hip"
M(3080, F, "cnt[(size_t)q * R + r] = c * m;", "cnt[(size_t)q * R + r] = c;", KFDB, "kfdb count: a key added twice counts its words once")
M(3081, F, "if (p >= 0) { c++; f = (unsigned)p < f ? (unsigned)p : f; }", "if (p >= 0) { c++; f = (unsigned)p; }", KFDB, "kfdb count: a lane keeps its last shared word's position, not its first")
M(3082, F, "if (tid == 0) start[base] = nvalid;", "if (tid == 0) start[base] = nvalid - 1;", VOC + KFDB[:1], "emit_runs: the last run ends one entry early")
M(3083, F, "if ((a > b2) == up) { key[t] = b2; key[p] = a; }", "if ((a >= b2) == up) { key[t] = b2; key[p] = a; }", VOC, "bitonic sort: equal keys are exchanged",
  note="equivalent: a real key carries its feature index in its low 16 bits, so two real keys never compare equal; the only equal keys are the kEmpty padding, and exchanging two equal values changes nothing")
M(3084, F, "if (i == 0) n_out[b] = nl + nr;", "if (i == 0) n_out[b] = nl;", ["test_rig_bow_batch.py", "test_keyframe_extracted.py"], "rig gather: the feature count forgets camera 2")

# ---- orbm_search.cpp: the resident map's host code ----
F = "orbm_search.cpp"
M(3100, F, "if (P || (m->state[slots[i]] & kMapPresent)) m->state[slots[i]] = st;", "", M_BUILD[:5] + M_SKIP[:2], "map scatter: the host mirror of `state` is not updated")
M(3101, F, "slot[(size_t)b * cap + j] = F.free_slots[j];\n            m->state[F.free_slots[j]] = (uint8_t)kMapPresent;", "slot[(size_t)b * cap + j] = F.free_slots[j];", M_STEREO,
  "stereo points: the host mirror does not learn of the new points")
M(3102, F, "for (int k = 0; k < i; k++) m->mark[slots[k]] = 0;", "for (int k = 0; k + 1 < i; k++) m->mark[slots[k]] = 0;", M_BUILD, "distinct slots: the mark of the last checked slot stays set")
M(3103, F, "if (p + n > max_positions) return fail(", "if (p + n >= max_positions) return fail(", M_BUILD, "local points: a walk of exactly the epoch's length refused")
M(3104, F, "if ((long long)m->base + L > (long long)m->epoch_limit) {", "if ((long long)m->base + L >= (long long)m->epoch_limit) {", M_BUILD, "local points: the stamps are cleared one build early", note=EARLY)
M(3105, F, "if (rt::memset_async(stamp, 0, 2 * pairs * sizeof(unsigned), h->s0)) return fail(ORBX_E_DEVICE, \"clearing the stamps failed: %s\", rt::last_error());\n        m->base = 0;", "m->base = 0;", M_BUILD,
  "local points: at the end of an epoch base starts over and the stamps stay")
M(3106, F, "m->base = top;  ", "", M_BUILD, "local points: base is not advanced")
M(3107, F, "seen_stamp, m->slots, base + 1u);", "seen_stamp, m->slots, base);", M_BUILD, "local points: the seen marks carry the previous call's value")
M(3108, F, "m->built[b] = 1;\n    return ORBX_OK;", "return ORBX_OK;", M_BUILD, "map_lay_set: built[b] is not set")
M(3109, F, "orbm_points& P = m->sets[b];\n    P.M = 0;", "orbm_points& P = m->sets[b];", M_BUILD + M_SKIP[1:2], "map_lay_set: P.M is left stale")
M(3110, F, "if (!(m->state[slots[i]] & kMapPresent)) return fail(ORBX_E_ARG, \"set %d: slot %d (entry %d) holds no point\", b, slots[i], i);", "", M_BUILD, "map select: a slot that holds nothing is accepted")
M(3111, F, "if (span < (long long)m->sets[s].M) return fail(", "if (span <= (long long)m->sets[s].M) return fail(", M_FLAGS[1:2] + ["test_state_gaps.py"], "sets fetch: a span that fits exactly refused")
M(3112, F, "for (int b = 0; b < B; b++) m->sets[b].M = 0;\n    if (L == 0) {", "if (L == 0) {", M_BUILD, "local points: the sets keep their old size while they are rebuilt",
  note="one of a redundant pair: map_lay_set sets P.M = 0 for every set the call rebuilds before anything is written into it (mutant 3109 is the other place), and a call refused in front "
       "of this line must leave the sets as they are (tests/test_map_scan_tiles.py); between this line and map_lay_set only a device failure returns")
# map_skip_table, fuse_map_run, orbm_map_edit_keyframes
M(3113, F, "} else if ((long long)m->tbase + M > (long long)m->epoch_limit) {", "} else if ((long long)m->tbase + M >= (long long)m->epoch_limit) {", M_SKIP, "skip table: cleared one call early", note=EARLY)
M(3114, F, "if (rt::memset_async(m->d_table.p, 0, bytes, h->s0)) return fail(ORBX_E_DEVICE, \"clearing the map's table failed: %s\", rt::last_error());\n        m->tbase = 0;", "m->tbase = 0;", M_SKIP,
  "skip table: at the end of an epoch tbase starts over and the table stays")
M(3115, F, "m->tbase = S->top;  ", "", M_SKIP, "skip table: tbase is not advanced")
M(3116, F, "if (f0 < 0 || (long long)f0 + N > n) return fail(", "if (f0 < 0 || (long long)f0 + N >= n) return fail(", M_SKIP, "fuse on the map: features that end exactly at the row's end refused")
M(3117, F, "if (keys[j].first == keys[j - 1].first)\n", "if (false)\n", M_SKIP[1:2], "edit key frames: two edits of one entry accepted")
M(3118, F, "for (int j = 1; j < n; j++)\n        if (keys[j].first == keys[j - 1].first)", "for (int j = 2; j < n; j++)\n        if (keys[j].first == keys[j - 1].first)", M_SKIP[1:2] + ["test_state_gaps.py"],
  "edit key frames: the two smallest entries are not compared")
# orbm_map_stereo_points
M(3120, F, "else if (cnt[2 * b] > frames[b].nfree) { refused = b; why = 1; }", "else if (cnt[2 * b] >= frames[b].nfree) { refused = b; why = 1; }", M_STEREO, "stereo points: exactly as many free slots as points refused")
M(3121, F, "else if (cnt[2 * b] > cap) { refused = b; why = 2; }", "else if (cnt[2 * b] >= cap) { refused = b; why = 2; }", M_STEREO, "stereo points: exactly cap points refused")
M(3122, F, "m->kf_n[F.row] = std::max(m->kf_n[F.row], nimg[F.frame]); m->kf_set[F.row] = 1; }", "m->kf_n[F.row] = std::max(m->kf_n[F.row], nimg[F.frame]); }", M_STEREO, "stereo points: the row a frame wrote does not count as set")
M(3123, F, "if (rows[r] == rows[r - 1]) return fail(ORBX_E_ARG, \"%s: row %d is named by two frames\", entry, rows[r]);", ";", M_STEREO, "stereo points: two frames may write one row")

# ---- orbv_api.cpp: the key frame database ----
F = "orbv_api.cpp"
M(3200, F, "if (i > 0 && id[i] <= id[i - 1]) return fail(", "if (i > 0 && id[i] < id[i - 1]) return fail(", KFDB, "kfdb add: a word id twice in one BowVector accepted")
M(3201, F, "if (it != db->keys.end() && (it->second.n != n || it->second.sum != sum))", "if (it != db->keys.end() && (it->second.n != n))", KFDB, "kfdb add: another BowVector of the same size under a live key accepted")
M(3202, F, "db->rlive[r] = 0; db->live--; db->dead_words += db->rn[r];", "db->rlive[r] = 0; db->live--;", KFDB, "kfdb erase: the erased words are not counted",
  note="equivalent in every output: dead_words only decides WHEN db_sync compacts the arena; an erased record carries the multiplicity 0 (db_sync builds `mult` from the keys' surviving records) "
       "and is passed over by k_kfdb_count whether it has been compacted away or not.  The arena then grows where it would have been compacted; what a compaction does is covered "
       "from the other side (3203, tests/test_kfdb_state.py)")
M(3203, F, "db->dead_words = 0; db->up_words = 0; db->meta_dirty = true;\n}", "db->dead_words = 0; db->meta_dirty = true;\n}", KFDB, "kfdb compact: the device keeps the arena prefix of before the compaction")
M(3205, F, "(size_t)db->dead_words > live_words)) db_compact(db);", "(size_t)db->dead_words >= live_words)) db_compact(db);", KFDB, "kfdb sync: compaction when the erased words EQUAL the live ones",
  note="equivalent in every output: a compaction keeps the surviving records in add order and changes no result (tests/test_kfdb_state.py queries on both sides of the threshold and requires the model's answer on both)")
M(3207, F, "mult[kv.second.recs.front()] = (int)kv.second.recs.size();", "mult[kv.second.recs.back()] = (int)kv.second.recs.size();", KFDB, "kfdb sync: the LAST surviving add of a key carries its count")
M(3208, F, "db_kill(db, it->second.recs.front());\n    it->second.recs.pop_front();", "db_kill(db, it->second.recs.back());\n    it->second.recs.pop_back();", KFDB, "kfdb erase: the latest add of the key goes, not the earliest")
M(3209, F, "if (it->second.recs.empty()) db->keys.erase(it);\n    return ORBX_OK;", "return ORBX_OK;", KFDB, "kfdb erase: a key without records is remembered with its BowVector")
M(3210, F, "for (int r : it->second.recs) db_kill(db, r);\n        db->keys.erase(it);", "db_kill(db, it->second.recs.front());\n        db->keys.erase(it);", KFDB, "kfdb erase_keys: only the first add of a key is counted as erased")
M(3211, F, "db->live = 0; db->dead_words = 0; db->up_words = 0; db->meta_dirty = true;\n    return ORBX_OK;", "db->live = 0; db->dead_words = 0; db->meta_dirty = true;\n    return ORBX_OK;", KFDB,
  "kfdb clear: the device keeps the arena prefix of before the clear")
M(3212, F, "!it->second.recs.empty()) xr.push_back(it->second.recs.front());", "!it->second.recs.empty()) xr.push_back(it->second.recs.back());", KFDB, "kfdb query: an exclusion names the key's latest add")
M(3213, F, "if (n > cap) too_small = 1;", "if (n >= cap) too_small = 1;", KFDB, "kfdb query: a result of exactly cap keys refused")
# orbm_distinctive_descriptors_resident, keyframes_from_records, map_row_check, fuse_pairs_finish, db_sync's growth
F = "orbm_search.cpp"
DIST_RES = ["test_state_gaps.py", "test_distinctive_resident.py"]
M(3130, F, "if (obs_start[p + 1] - obs_start[p] > kDistinctiveMax)", "if (obs_start[p + 1] - obs_start[p] >= kDistinctiveMax)", DIST_RES, "distinctive (resident): a point with exactly the most observations allowed refused")
M(3133, F, "for (int q = 0; q < p; q++) if (slots[q] >= 0 && slots[q] < map->slots) map->mark[slots[q]] = 0;", "for (int q = 0; q + 1 < p; q++) if (slots[q] >= 0 && slots[q] < map->slots) map->mark[slots[q]] = 0;", DIST_RES,
  "distinctive (resident): the mark of the last checked slot stays set")
M(3134, F, "recs.push_back({writes && slots[p] >= 0 ? map->S.desc", "recs.push_back({writes && slots[p] > 0 ? map->S.desc", DIST_RES, "distinctive (resident): the winner of the point at slot 0 is not written into the map")
M(3135, F, "if (n == 0 || (n > kDistinctiveRegMax) != (form == 1)) continue;", "if (n == 0 || (n >= kDistinctiveRegMax) != (form == 1)) continue;", DIST_RES, "distinctive (resident): a point of exactly kDistinctiveRegMax observations takes the LDS form",
  note="equivalent in every output: the two forms of k_distinctive_resident differ in where a point's distance rows are kept (registers up to kDistinctiveRegMax observations, LDS "
       "beyond - the LDS of the launch is sized by the largest n of the call either way), not in what they compute: the same distinctive_point<kLds> body, the same medians, the same "
       "first-minimum rule; tests/test_distinctive_resident.py requires its expected choice of points with 63, 64 and 65 observations, on either side of the line")
M(3141, F, "a0 += (size_t)kf->N;\n    }\n    for (int j = 0; j < n; j++) out[j] = made[j];", "}\n    for (int j = 0; j < n; j++) out[j] = made[j];", M_KF, "key frames from records: every key frame gets the first one's keypoint angles")
M(3150, F, "if (K->N != m->kf_n[row]) return fail(", "if (K->N > m->kf_n[row]) return fail(", M_ROWS + ["test_state_gaps.py"], "map row check: a row longer than its key frame accepted")
M(3155, F, "if (total > (size_t)W.cap) return fail(ORBX_E_CAPACITY, \"%zu pairs do not fit in cap = %d\", total, W.cap);", "if (total >= (size_t)W.cap) return fail(ORBX_E_CAPACITY, \"%zu pairs do not fit in cap = %d\", total, W.cap);", PAIRS,
  "fuse pairs: a list of exactly cap pairs refused")
F = "orbv_api.cpp"
M(3217, F, "db->up_words = 0;\n    }\n    if (R > db->d_rn.n) {", "}\n    if (R > db->d_rn.n) {", KFDB, "kfdb sync: a grown arena keeps only the appended tail")
# check_capacity (the extractor's capacity, at both of its call sites through run()), batch_fetch, an empty set in the pair-list Fuse
F = "orbv_api.cpp"
M(3218, F, "if (cap > 16384) return fail(ORBX_E_CAPACITY, \"more than 16384 features per image\");", "if (cap >= 16384) return fail(ORBX_E_CAPACITY, \"more than 16384 features per image\");",
  ["test_kfdb_state.py", "test_emu_vocab.py", "test_rig_bow_batch.py"], "check_capacity: an extractor of exactly 16384 key points refused")
F = "orbm_search.cpp"
M(3156, F, "if (M == 0) { if (want) std::fill(want->start, want->start + K + 1, 0); return ORBX_OK; }", "if (M == 0) { return ORBX_OK; }", PAIRS + M_SKIP[1:2], "fuse pairs: an empty point set leaves `start` as the caller's array held it")
M(3157, F, "memcpy(views[v] + b * M1, src, m); memset(views[v] + b * M1 + m, 0, M1 - m);", "memcpy(views[v] + b * M1, src, m);", ["test_local_points_maps.py", "test_local_map_search.py", "test_local_map_build.py::test_searches_emulated"],
  "batch fetch: mbTrackInView behind a frame's own points is not zeroed")
