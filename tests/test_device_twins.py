"""Every test that runs the kernel sources on the SIMT emulator (it takes the `emu_lib` fixture) has a form that runs on the device, or says why not.

The emulator cannot see what only the device does: rt::check_launch() is `return 0` there (a zero-sized grid or an LDS request over the limit is
legal), its workgroups are fibers (no real concurrency behind the candidate pool's atomicAdd), and plain C stands in for the SDWA ballots, v_mbcnt
ranks and packed binary16 scores of k_fast_cells.  So an edge case that exists for the emulator alone is an edge case nobody has run.

This file reads the test files with `ast` and imports nothing of the library.  A device twin of tests/test_x.py::test_y(emu_lib) is, in this order,
  1. named in TWINS below (the device form has another name, or several tests share one device form);
  2. found by name: test_y with its `_emulated` / `_emulator` suffix replaced by `_gpu` (or `_gpu` appended), or `test_gpu_` in front, in any file;
     or the same name in the `test_gpu_` file that goes with a `test_emu_` file;
  3. found by helper: the body of test_y is nothing but `helper(emu_lib, ..)`, and a device test calls the same helper.
A device test takes `hip_lib` and carries the gpu mark (its own, or the module's `pytestmark`).
Everything else must be in EXEMPT with a one-line reason.  The test fails on an emulator-only test that is neither, on a TWINS entry whose
device form is gone, and on a TWINS / EXEMPT entry whose test no longer exists."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))

# emulator test -> its device form(s), where the names do not say it
TWINS = {
    "test_emu_parity.py::test_extractor_stagewise_and_final": ["test_gpu_parity.py::test_extractor_vs_oracle", "test_gpu_parity.py::test_stagewise_full_size"],
    "test_emu_parity.py::test_empty_image_and_errors": ["test_gpu_parity.py::test_empty_and_errors"],
    "test_emu_parity.py::test_batch_and_stereo_and_knn": ["test_gpu_parity.py::test_stereo_full_size_batch", "test_gpu_parity.py::test_fisheye_knn_ratio",
                                                          "test_gpu_parity.py::test_hamming_matrix"],
    "test_emu_parity.py::test_knn_ties_and_degenerate_sizes": ["test_gpu_parity.py::test_hamming_matrix"],
    "test_emu_parity.py::test_two_extractor_instances_concurrently": ["test_gpu_parity.py::test_two_instances_on_two_threads"],
    "test_emu_parity.py::test_golden_fixture": ["test_gpu_parity.py::test_golden_fixtures"],
    "test_emu_fuzz.py::test_fuzz": ["test_gpu_parity.py::test_fuzz_gpu"],
    "test_emu_search.py::test_guided_searches_emulated": ["test_gpu_search.py::test_guided_searches_gpu_full_size", "test_gpu_search.py::test_guided_searches_gpu_euroc_size"],
    "test_emu_mappoint.py::test_distinctive_descriptors_emulated": ["test_gpu_search.py::test_distinctive_descriptors_gpu"],
    "test_emu_kfdb.py::test_kfdb_extracted_emulated": ["test_gpu_kfdb.py::test_kfdb_scale_gpu"],
    "test_emu_kfdb.py::test_kfdb_numpy_restatement_emulated": ["test_gpu_kfdb.py::test_kfdb_scale_gpu"],
    "test_emu_pyramid_export.py::test_export_equals_reflect101_frames": ["test_gpu_pyramid_export.py::test_gpu_export_equals_reflect101_frames"],
    "test_emu_pyramid_export.py::test_export_euroc_752x480": ["test_gpu_pyramid_export.py::test_gpu_export_equals_reflect101_frames"],
    "test_emu_pyramid_export.py::test_edge_wider_than_the_smallest_level": ["test_gpu_pyramid_export.py::test_gpu_export_sizes_edges_and_inputs"],
    "test_emu_pyramid_export.py::test_live_resources_return_to_zero": ["test_gpu_pyramid_export.py::test_gpu_live_resources_return"],
    "test_mono_init.py::test_pool_form_takes_30000_features_emulated": ["test_mono_init.py::test_pool_form_takes_64000_features_gpu"],
    "test_gpu_headline_shape.py::test_headline_shape_emulated": ["test_gpu_headline_shape.py::test_headline_shape_stereo_gpu"],
    "test_rig_tracking_batch.py::test_rig_batch_local_points_two_handles_emulated": ["test_rig_tracking_batch.py::test_rig_batch_two_handles_gpu"],
    "test_rig_tracking_batch.py::test_rig_batch_lastframe_two_handles_emulated": ["test_rig_tracking_batch.py::test_rig_batch_two_handles_gpu"],
    # (properties of the scene, counted on the oracle; the single-call projection in front of it is the one test_parity_gpu makes for the same scene)
    "test_fuse_batch.py::test_scene_conditions_hold_on_the_oracle": ["test_fuse_batch.py::test_parity_gpu"],
    "test_sim3_projection_batch.py::test_scene_conditions_hold_on_the_oracle": ["test_sim3_projection_batch.py::test_parity_gpu"],
    "test_bench_dist.py::test_bench_two_ranks_gloo": ["test_bench_dist.py::test_bench_two_ranks_share_one_gpu"],
    "test_bench_dist.py::test_bench_launches_its_own_ranks": ["test_bench_dist.py::test_bench_four_ranks_share_one_gpu_in_16_cores"],
}

# emulator tests that stay emulator-only, and why
EXEMPT = {
    "test_abi.py::test_null_arguments_are_refused_not_dereferenced": "argument refusals: null pointers and zero sizes never reach a launch",
    "test_emu_fuzz.py::test_portrait_aspect_is_rejected_like_the_reference_would_crash": "argument refusal: the aspect ratio is refused before anything is launched",
    "test_emu_input.py::test_input_error_paths": "argument refusals (channel count, stride) that never reach a launch",
    "test_emu_kfdb.py::test_kfdb_scores_need_the_oracle": "checks the reference scorer the other tests compare with; the library computes nothing in it",
    "test_emu_kfdb.py::test_kfdb_kl_refused": "argument refusal: the KL scoring is refused when the database is created",
    "test_emu_parity.py::test_feature_counts_beyond_the_lds_take_the_node_pool": "needs ORBX_EMU_LDS_LIMIT (the device's own limit: test_mono_init.py, the _gpu pool-form tests)",
    "test_emu_pyramid_export.py::test_stale_or_out_of_range_image_is_refused": "argument refusals of orbx_pyramid_exported: a host check of the slot's generation, no launch",
    "test_emu_pyramid_export.py::test_bad_settings_are_refused": "argument refusals of orbx_set_pyramid_export that never reach a launch",
    "test_emu_search.py::test_round3_entry_points_reject_bad_arguments": "argument refusals of the batched entry points that never reach a launch",
    "test_emu_vocab.py::test_vocabulary_error_paths": "argument refusals and malformed vocabulary files: host parsing, no launch",
    "test_kfdb_reference.py::test_restatement_reference_and_facade_agree": "pins the restatement on the reference's own KeyFrameDatabase.cc, a CPU library; the facade's answers on the same constructed scenarios have their device form in test_kfdb_gates.py::test_kfdb_gates_gpu",
    "test_facade.py::test_vocabulary_facade_emulated": "compiles the reference's DBoW2 sources at test time, which the device box does not have (device: test_gpu_vocab.py)",
    "test_facade.py::test_facade_headers_link_from_several_translation_units": "a link test of the headers: the program constructs a matcher and launches nothing",
    "test_lifetime.py::test_failed_calls_hold_nothing": "argument refusals: what a refused create / extract / selftest leaves allocated, no launch",
    "test_mono_init.py::test_pool_form_is_what_the_big_settings_take": "needs ORBX_EMU_LDS_LIMIT",
    "test_multi_comm.py::test_allgather_two_ranks_emulated": "two ranks on the emulator's two devices; the device box admits one GPU (device, one rank: test_allgather_one_rank_rccl_gpu)",
    "test_multi_gloo.py::test_two_ranks_gloo": "a gloo world of two ranks on the emulator's two devices; the device box admits one GPU (device: test_multi_comm.py)",
    "test_bench_dist.py::test_bench_eight_ranks_gloo": "gloo world size 8: the device box does not admit eight processes with the GPU open",
    "test_bench_dist.py::test_bench_plain_run_times_its_steps_and_dumps_outputs": "bench.py's own timing and dump bookkeeping, host code; the device runs bench.py in test_bench_two_ranks_share_one_gpu",
    "test_bench_dist.py::test_bench_dump_other_configs": "bench.py's dump of the other configurations, host code; the device runs bench.py in test_bench_two_ranks_share_one_gpu",
    "test_rig_bow_batch.py::test_rig_bow_refusals_emulated": "argument refusals of the rig BoW entry points that never reach a launch",
    "test_rig_tracking_batch.py::test_rig_batch_refusals_emulated": "argument refusals and the one-pending-batch rule, host checks (device: test_pending_batch.py::test_pending_batch_gpu)",
    "test_undistort.py::test_model_change_after_extraction_is_refused": "argument refusal: a stale undistortion model is refused before the search is enqueued",
}


def _gpu_marked(fn, module_gpu):
    return module_gpu or any("mark.gpu" in ast.unparse(d) for d in fn.decorator_list)


def _calls(fn):
    return {ast.unparse(c.func) for c in ast.walk(fn) if isinstance(c, ast.Call)}


def _only_helper(fn):
    """the helper's name when the body is a docstring at most and one expression `helper(emu_lib, ..)`"""
    body = [s for s in fn.body if not (isinstance(s, ast.Expr) and isinstance(s.value, ast.Constant) and isinstance(s.value.value, str))]
    if len(body) != 1 or not isinstance(body[0], ast.Expr) or not isinstance(body[0].value, ast.Call):
        return None
    call = body[0].value
    if not any(isinstance(a, ast.Name) and a.id == "emu_lib" for a in call.args):
        return None
    return ast.unparse(call.func).split(".")[-1]


def collect(paths):
    """({id: function} of the emulator tests, {id: function} of the device tests, every test id)"""
    emu, dev, every = {}, {}, set()
    for path in paths:
        tree = ast.parse(open(path).read())
        name = os.path.basename(path)
        module_gpu = any(isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "pytestmark" for t in n.targets) and "mark.gpu" in ast.unparse(n.value)
                         for n in tree.body)
        for fn in tree.body:
            if isinstance(fn, ast.FunctionDef) and fn.name.startswith("test"):
                args = [a.arg for a in fn.args.args]
                every.add(name + "::" + fn.name)
                if "emu_lib" in args:
                    emu[name + "::" + fn.name] = fn
                if "hip_lib" in args and _gpu_marked(fn, module_gpu):
                    dev[name + "::" + fn.name] = fn
    return emu, dev, every


def twin_of(tid, fn, dev):
    """the device form found by the conventions, or None"""
    fname, name = tid.split("::")
    base = name
    for suffix in ("_emulated", "_emulator"):
        if name.endswith(suffix):
            base = name[:-len(suffix)]
    wanted = {base + "_gpu", base.replace("test_", "test_gpu_", 1)}
    for d in dev:
        if d.split("::")[1] in wanted:
            return d
    if fname.startswith("test_emu_") and fname.replace("test_emu_", "test_gpu_", 1) + "::" + name in dev:
        return fname.replace("test_emu_", "test_gpu_", 1) + "::" + name
    helper = _only_helper(fn)
    if helper:
        for d, dfn in dev.items():
            if any(c.split(".")[-1] == helper for c in _calls(dfn)):
                return d
    return None


def audit(emu, dev, every, twins, exempt):
    """the list of complaints; empty when every emulator test is accounted for"""
    out = []
    for tid, forms in twins.items():
        if tid not in emu:
            out.append("TWINS names %s, which is no emulator test (any more)" % tid)
        out += ["TWINS: the device form %s of %s does not exist or is not a gpu-marked test with hip_lib" % (d, tid) for d in forms if d not in dev]
    for tid in exempt:
        if tid not in every:
            out.append("EXEMPT names %s, which no longer exists" % tid)
        elif tid not in emu:
            out.append("EXEMPT names %s, which does not take emu_lib" % tid)
        if tid in twins:
            out.append("%s is both in TWINS and in EXEMPT" % tid)
    for tid, fn in sorted(emu.items()):
        if tid in twins or tid in exempt:
            continue
        if twin_of(tid, fn, dev) is None:
            out.append("%s runs on the emulator only: give it a device form (a helper that takes the library, called from a gpu-marked test with hip_lib), "
                       "or name its device form in TWINS, or say in EXEMPT why it has none" % tid)
    return out


def _test_files():
    return sorted(glob.glob(os.path.join(HERE, "test_*.py")))


def test_every_emulator_test_has_a_device_twin_or_a_reason():
    emu, dev, every = collect(_test_files())
    assert len(emu) > 150 and len(dev) > 150, "the scan found %d emulator tests and %d device tests: it does not see the suite" % (len(emu), len(dev))
    problems = audit(emu, dev, every, TWINS, EXEMPT)
    assert not problems, "\n".join(problems)
    assert all(len(reason) > 20 and "\n" not in reason for reason in EXEMPT.values())


def test_the_audit_notices(tmp_path):
    """the audit on a suite made for it: one test of each kind"""
    (tmp_path / "test_emu_thing.py").write_text(
        "import pytest\n"
        "def _case(lib, n): pass\n"
        "def test_named_emulated(emu_lib): x = 1\n"
        "def test_same_name(emu_lib): x = 1\n"
        "def test_by_helper(emu_lib):\n    '''doc'''\n    _case(emu_lib, 3)\n"
        "def test_mapped(emu_lib): x = 1\n"
        "def test_excused(emu_lib): x = 1\n"
        "def test_alone(emu_lib): x = 1\n"
        "def test_helper_and_more(emu_lib):\n    _case(emu_lib, 3)\n    assert True\n"
        "def test_cpu_only(): pass\n")
    (tmp_path / "test_gpu_thing.py").write_text(
        "import pytest\nfrom test_emu_thing import _case\npytestmark = pytest.mark.gpu\n"
        "def test_same_name(hip_lib): pass\n"
        "def test_other(hip_lib): _case(hip_lib, 5)\n"
        "def test_elsewhere(hip_lib): pass\n")
    (tmp_path / "test_mixed.py").write_text(
        "import pytest\n"
        "@pytest.mark.gpu\ndef test_named_gpu(hip_lib): pass\n"
        "def test_alone_gpu(hip_lib): pass\n")                      # no gpu mark: not a device form
    emu, dev, every = collect(sorted(glob.glob(str(tmp_path / "test_*.py"))))
    twins = {"test_emu_thing.py::test_mapped": ["test_gpu_thing.py::test_elsewhere"]}
    exempt = {"test_emu_thing.py::test_excused": "argument refusals that never reach a launch"}
    got = audit(emu, dev, every, twins, exempt)
    assert len(got) == 2 and "test_alone runs on the emulator only" in got[0] and "test_helper_and_more runs on the emulator only" in got[1], got
    # a device form that went away, an exemption whose test went away, one for a test that is no emulator test
    got = audit(emu, dev, every, {"test_emu_thing.py::test_mapped": ["test_gpu_thing.py::test_gone"]},
                dict(exempt, **{"test_emu_thing.py::test_removed": "argument refusals that never reach a launch", "test_emu_thing.py::test_cpu_only": "it never takes the library"}))
    assert sum("test_gone" in g for g in got) == 1 and sum("test_removed, which no longer exists" in g for g in got) == 1
    assert sum("test_cpu_only, which does not take emu_lib" in g for g in got) == 1 and len(got) == 5, got
