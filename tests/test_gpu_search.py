"""Guided searches on the real GPU at BASELINE.json config-4 sizes (640x480, nFeatures=1000, 5000 map points)."""
import numpy as np
import pytest

from test_emu_search import degenerate_views, run_all
from test_emu_search_fuzz import CROWDED_CASES, FUZZ_SEEDS, grid_build_crowded_cells, projection_searches_fuzz

pytestmark = pytest.mark.gpu


def test_guided_searches_gpu_full_size(hip_lib):
    run_all(None, 640, 480, 1000, 5000, seeds=(0, 1, 2))


def test_guided_searches_gpu_euroc_size(hip_lib):
    run_all(None, 752, 480, 1200, 3000, seeds=(5,))


def test_distinctive_descriptors_gpu(hip_lib):
    from test_emu_mappoint import run
    run(None, 5000, 60, 2)          # config-4 scale: ~5000 local map points
    run(None, 200, 400, 3)


def test_matchers_from_three_threads_gpu(hip_lib):
    from test_emu_search import concurrent_matchers
    concurrent_matchers(None, 640, 480, 1000, 3000)


def test_degenerate_views(hip_lib):
    degenerate_views(hip_lib)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_projection_searches_fuzz(hip_lib, seed):
    """random thresholds and occupancies at the emulator's shapes; seed 5 is an empty frame, the point sets include sizes 0 and 1"""
    projection_searches_fuzz(hip_lib, seed)


@pytest.mark.parametrize("clusters,N", CROWDED_CASES)
def test_grid_build_crowded_cells(hip_lib, clusters, N):
    grid_build_crowded_cells(hip_lib, clusters, N)
