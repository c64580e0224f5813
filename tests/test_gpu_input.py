"""Input pre-step on the real GPU at EuRoC size (752x480: rectification, 600x350 resize, colour frames)."""
import pytest

from test_emu_input import run

pytestmark = pytest.mark.gpu


def test_input_prestep_gpu(hip_lib):
    run(None, 752, 480, 1200)


def test_input_prestep_odd_width_gpu(hip_lib):
    """the emulator's odd shape (3 x 483 bytes per row, 361 rows): the partial last group of k_input_gray's rows on the device"""
    run(hip_lib, 483, 361, 500)
