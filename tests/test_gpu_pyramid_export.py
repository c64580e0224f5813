"""Bordered pyramid export on the MI355X (liborbx_hip.so): k_frame_pyramid's frames against the numpy restatement of copyMakeBorder(REFLECT_101)
at B = 1, 3 and 8, under graph replay, across the ring and the other input paths; and the reference's unchanged stereo Frame constructor on the
drop-in extractor for consecutive pairs (the facade reads mvImagePyramid from the export ring)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import pyramid_export_check as pc
from orb_slam3_detailed_comments_amd import synth, _lib
from orb_slam3_detailed_comments_amd.extractor import ORBextractor
from test_emu_pyramid_export import (export_off_by_default_allocates_nothing, exported_arrays_are_views_of_the_slot, input_pre_step_and_on_device_frames, other_scale_and_levels, ring_keeps_older_exports, toggle_reconfigure_and_batch_growth)

pytestmark = pytest.mark.gpu

DROPIN = os.path.join(ol.ROOT, "oracle", "_ref", "libref_frame_dropin.so")


def _batch(B, w=752, h=480, seed=0):
    return np.stack([synth.corner_field(w, h, seed=seed + b) if b % 3 else synth.natural(w, h, seed=seed + b) for b in range(B)])


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("graph", [False, True])
def test_gpu_export_equals_reflect101_frames(hip_lib, B, graph):
    ex = ORBextractor(1200, 1.2, 8, 20, 7, lib=hip_lib)
    ex.pyramid_export(19, 2)
    ex.graph_replay(graph)
    seq = [_batch(B, seed=10 * k) for k in range(4)]       # the ring: the previous extraction's views stay intact (replays reuse one graph)
    held = pc.ring_check(ex, seq, 19, 2, B)
    n_plain = [len(r[1]) for r in ex.extract_batch(seq[-1])]
    pc.check_export(ex, B, 19)
    ex.pyramid_export(0)                                    # the keypoints do not depend on the export
    assert [len(r[1]) for r in ex.extract_batch(seq[-1])] == n_plain
    assert len(held) == 4
    ex.close()


def test_gpu_export_sizes_edges_and_inputs(hip_lib):
    for w, h, nf, edge in ((239, 239, 1000, 100), (477, 239, 100, 19), (1241, 376, 2000, 19), (376, 240, 500, 33)):
        ex = ORBextractor(nf, 1.2, 8, 20, 7, lib=hip_lib)
        ex.pyramid_export(edge, 3)
        ex.extract_batch(np.stack([synth.uniform_noise(w, h, seed=1), synth.corner_field(w, h, seed=2, nrect=500)]))
        pc.check_export(ex, 2, edge)
        ex.close()
    # frames written into level 0 (on_device) and a colour + resize pre-step, with a geometry change in between
    ex = ORBextractor(1200, 1.2, 8, 20, 7, lib=hip_lib)
    ex.pyramid_export(19, 2)
    imgs = _batch(3, seed=40)
    p, shape, st, ist = ex.input_upload(imgs)
    ex.enqueue(None, device_ptr=p, shape=shape, stride=st, image_stride=ist); ex.fetch()
    pc.check_export(ex, 3, 19)
    ex.set_input(channels=3, rgb=True, resize=(640, 480))
    ex.extract_batch(np.repeat(_batch(2, seed=50)[..., None], 3, axis=3))
    pc.check_export(ex, 2, 19)
    ex.close()


def test_gpu_live_resources_return(hip_lib):
    base = pc.live(hip_lib)
    ex = ORBextractor(1200, 1.2, 8, 20, 7, lib=hip_lib)
    ex.pyramid_export(19, 2)
    ex.extract_batch(_batch(2))
    ex.exported_pyramid(1)
    ex.sync()
    ex.close()
    assert np.array_equal(pc.live(hip_lib), base)


@pytest.mark.skipif(not os.path.exists(DROPIN), reason="oracle/_ref/libref_frame_dropin.so not built")
def test_gpu_reference_frame_repeat_on_dropin(hip_lib):
    """ref_frame_stereo_repeat: one pair of drop-in extractors, a new reference Frame per stereo pair for at least 20 pairs; the last pair's
    stereo match count equals the all-reference build's (libref_frame.so)."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ol.ROOT, os.path.join(ol.ROOT, "tests")]))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ol.ROOT, "tests", "dropin_repeat_runner.py"), _lib.HIP_LIB_PATH,
                        "752", "480", "100", "0.25"], capture_output=True, text=True, env=env, timeout=320)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["frames"] >= 20, got
    left, right = synth.stereo_pair(752, 480, seed=100)
    n, _, m_ref, _, _ = ol.reference_frame_repeat(left, right, 0.0)
    assert n == 1 and got["matches"] == m_ref and m_ref > 100, (got, m_ref)


def test_gpu_other_scale_and_levels(hip_lib):
    other_scale_and_levels(hip_lib)


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_gpu_ring_keeps_depth_minus_one_older_exports(hip_lib, depth):
    ring_keeps_older_exports(hip_lib, depth)


def test_gpu_toggle_reconfigure_and_batch_growth(hip_lib):
    toggle_reconfigure_and_batch_growth(hip_lib)


def test_gpu_input_pre_step_and_on_device_frames(hip_lib):
    input_pre_step_and_on_device_frames(hip_lib)


def test_gpu_export_off_by_default_allocates_nothing(hip_lib):
    export_off_by_default_allocates_nothing(hip_lib)


def test_gpu_exported_arrays_are_views_of_the_slot(hip_lib):
    exported_arrays_are_views_of_the_slot(hip_lib)
