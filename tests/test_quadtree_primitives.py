"""The workgroup primitives of csrc/k_quadtree.hip, run directly (orbx_debug_quadtree_selftest) on the inputs that images do not produce.

block_sort_libstdcxx - the parallel restatement of libstdc++'s std::sort that orders the nodes of the quadtree's final rounds - against the
real std::sort (tests/cpp/std_sort_helper.cpp, compiled here): full-array bit equality on keys count << 32 | x0 << 16 | index with the comparator
on key >> 16, so every difference in the tie permutation shows.  The inputs are ordinary std::sort adversaries; whether an input reaches the
heap-sort fallback is asserted from the helper's own count, never from the kernel.  block_partition4 against a numpy stable partition, with the
destination outside the span checked for being untouched; block_excl_scan_n against numpy.cumsum on 4 and 16 waves.

Every test has an emulator form and a GPU form on the same inputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from orb_slam3_detailed_comments_amd.extractor import ORBextractor

ROOT = ol.ROOT
CSRC = os.path.join(ROOT, "orb_slam3_detailed_comments_amd", "csrc")

SIZES = (0, 1, 2, 15, 16, 17, 18, 33, 63, 64, 65, 100, 127, 128, 129, 257, 1000, 4095)
SIZES_POOL_ONLY = (4096, 10000, 65535)             # beyond the 12-bit positions of the LDS form
FAMILIES = ("ties", "equal", "ascending", "descending", "organ_pipe", "two_values", "sawtooth17", "musser_killer", "mcilroy_adversary",
            "random1", "random2", "random3")
THREADS = (256, 1024)                               # the two values of LevelInfo::qt_threads


class StdSort:
    """tests/cpp/std_sort_helper.cpp behind ctypes"""

    def __init__(self, so):
        L = self.L = C.CDLL(so)
        L.qsh_std_sort.argtypes = [C.c_void_p, C.c_int]; L.qsh_std_sort.restype = None
        L.qsh_mcilroy_adversary.argtypes = [C.c_void_p, C.c_int]; L.qsh_mcilroy_adversary.restype = None
        L.qsh_musser_killer.argtypes = [C.c_void_p, C.c_int]; L.qsh_musser_killer.restype = None
        L.qsh_heap_ranges.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]; L.qsh_heap_ranges.restype = None
        self._cases = {}

    def sort(self, keys):
        out = np.ascontiguousarray(keys, np.uint64).copy()
        self.L.qsh_std_sort(out.ctypes.data, len(out))
        return out

    def heap_ranges(self, keys):
        keys = np.ascontiguousarray(keys, np.uint64)
        nr, ne = C.c_int(), C.c_longlong()
        self.L.qsh_heap_ranges(keys.ctypes.data, len(keys), C.byref(nr), C.byref(ne))
        return nr.value, ne.value

    def counts(self, family, n):
        a = np.zeros(max(n, 1), np.int32)
        (self.L.qsh_mcilroy_adversary if family == "mcilroy_adversary" else self.L.qsh_musser_killer)(a.ctypes.data, n)
        return a[:n].astype(np.uint64)

    def case(self, family, n):
        """(keys, std::sort of them, (heap-sorted ranges, their elements)); computed once per session"""
        if (family, n) not in self._cases:
            keys = make_keys(self, family, n)
            keys.setflags(write=False)
            exp = self.sort(keys)
            exp.setflags(write=False)
            self._cases[family, n] = (keys, exp, self.heap_ranges(keys))
        return self._cases[family, n]


def make_keys(std, family, n):
    i = np.arange(n, dtype=np.uint64)
    x0 = np.zeros(n, np.uint64)
    if family == "ties":                             # the (count, x0) distributions of the real final rounds
        rng = np.random.default_rng(1000 + n)
        cnt = rng.integers(2, 5, n).astype(np.uint64); x0 = (rng.integers(0, 4, n) * 90).astype(np.uint64)
    elif family == "equal":
        cnt = np.full(n, 5, np.uint64); x0 = np.full(n, 7, np.uint64)
    elif family == "ascending":
        cnt = i.copy()
    elif family == "descending":
        cnt = np.uint64(n) - i
    elif family == "organ_pipe":
        cnt = np.minimum(i, np.uint64(max(n, 1) - 1) - i)
    elif family == "two_values":
        cnt = np.random.default_rng(2000 + n).integers(0, 2, n).astype(np.uint64)
    elif family == "sawtooth17":
        cnt = i % np.uint64(17)
    elif family in ("musser_killer", "mcilroy_adversary"):
        cnt = std.counts(family, n)
    else:
        rng = np.random.default_rng(3000 * int(family[-1]) + n)
        cnt = rng.integers(2, 41, n).astype(np.uint64); x0 = rng.integers(0, 720, n).astype(np.uint64)
    return (cnt << np.uint64(32)) | (x0 << np.uint64(16)) | i


@pytest.fixture(scope="module")
def std(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("std_sort") / "libstd_sort_helper.so")
    subprocess.run(["g++", "-O2", "-std=c++14", "-shared", "-fPIC", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "std_sort_helper.cpp"), "-o", so], check=True)
    return StdSort(so)


def _extractor(lib):
    return ORBextractor(500, 1.2, 8, 20, 7, lib=lib)


# ---- the sort ---------------------------------------------------------------------------------------------------------------------------

def test_adversaries_reach_the_heap_fallback(std):
    """the figures the sort tests rest on, from the reference side: where the two adversaries first exhaust std::sort's depth budget"""
    assert std.case("musser_killer", 100)[2] == (1, 30)
    assert std.case("musser_killer", 4095)[2] == (22, 3062)
    assert std.case("mcilroy_adversary", 64)[2] == (1, 40)
    assert std.case("mcilroy_adversary", 4095)[2] == (1, 4051)
    assert std.case("mcilroy_adversary", 65535)[2] == (1, 65475)
    for n in (64, 1000):                              # the adversary's values are a permutation: no ties, one possible result
        k = std.case("mcilroy_adversary", n)[0]
        assert np.array_equal(np.sort(k >> np.uint64(32)), np.arange(n, dtype=np.uint64))


# (form, sizes): the LDS form and the node-pool form up to the 12-bit limit of the first, the pool form beyond it
SORT_CASES = [pytest.param(0, SIZES, id="lds"), pytest.param(1, SIZES, id="pool")] + [pytest.param(1, (n,), id="pool_%d" % n) for n in SIZES_POOL_ONLY]


def _check_sort(lib, std, spill, sizes, threads):
    ex = _extractor(lib)
    heap_cases = 0
    for n in sizes:
        for family in FAMILIES:
            keys, exp, (nranges, nelems) = std.case(family, n)
            # the branch this input is here for, by the reference's own count
            if family == "musser_killer":
                assert nranges >= 1 or n < 100, (family, n, nranges)
                if n == 4095: assert nranges > 1        # several threads heap-sort at the same time
            elif family == "mcilroy_adversary":
                assert nranges >= 1 or n < 64, (family, n, nranges)
            elif family == "organ_pipe":
                # libstdc++'s median-of-3 meets its worst case here as well (the real std::sort heap-sorts 1 range of 23 at n = 127, 14 ranges at 4095,
                # 57 at 65535): the one family besides the two adversaries that takes the fallback, and it takes it with tied counts
                assert (nranges >= 1) == (n in (127, 128, 257) or n >= 1000), (family, n, nranges)
            else:
                assert nranges == 0, (family, n, nranges)
            heap_cases += nranges > 0
            got = ex.debug_quadtree_sort(keys, spill, threads)
            if not np.array_equal(got, exp):
                bad = np.flatnonzero(got != exp)
                pytest.fail("%s, n = %d, spill = %d, %d threads (%d heap-sorted ranges of %d elements): %d positions differ from std::sort, the first at %d: %#x, expected %#x"
                            % (family, n, spill, threads, nranges, nelems, len(bad), bad[0], got[bad[0]], exp[bad[0]]))
    assert heap_cases >= (21 if sizes is SIZES else 3)
    ex.close()


@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("spill,sizes", SORT_CASES)
def test_sort_emulated(emu_lib, std, spill, sizes, threads):
    _check_sort(emu_lib, std, spill, sizes, threads)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
@pytest.mark.parametrize("spill,sizes", SORT_CASES)
def test_sort_gpu(hip_lib, std, spill, sizes, threads):
    _check_sort(hip_lib, std, spill, sizes, threads)


def test_sort_emulated_one_thread_ranges(tmp_path, std):
    """Ranges of up to kWaveSortRange elements are partitioned by one thread instead of a wave; with the product's value, 16, no range is that short (a
    range of 16 is final).  A build with 40 - one of the values tests/test_emu_variants.py runs images through - sends the ranges of 17 .. 40 elements
    there, in both forms of the range lists.  CPU only: a GPU build with another constant is a minute of compilation."""
    from test_emu_variants import build_emu_variant
    from orb_slam3_detailed_comments_amd import _lib
    so = str(tmp_path / "liborbx_emu_sortrange.so")
    build_emu_variant(so, ["-DORBX_WAVE_SORT_RANGE=40"])
    lib = _lib.OrbxLib(so)
    for spill in (0, 1):
        _check_sort(lib, std, spill, SIZES, 256)


def _check_sort_refusals(lib, std):
    ex = _extractor(lib)
    keys = std.case("ties", 4096)[0]
    out = np.zeros(4096, np.uint64)
    f = lib.L.orbx_debug_quadtree_selftest
    assert f(ex._h, 0, 0, 256, keys.ctypes.data, 4096, 0, 0, 0, 0, out.ctypes.data) == -2          # ORBX_E_ARG: 12-bit positions
    assert f(ex._h, 0, 1, 256, keys.ctypes.data, 65536, 0, 0, 0, 0, out.ctypes.data) == -2
    assert f(ex._h, 0, 1, 512, keys.ctypes.data, 100, 0, 0, 0, 0, out.ctypes.data) == -2           # not a size a tree runs on
    assert f(ex._h, 1, 0, 256, keys.ctypes.data, 100, 0, 200, 5, 5, out.ctypes.data) == -2         # a span that starts at 0
    assert f(ex._h, 1, 0, 256, keys.ctypes.data, 100, 101, 200, 5, 5, out.ctypes.data) == -2       # a span that leaves the buffer
    assert not out.any()
    ex.close()


def test_selftest_refusals_emulated(emu_lib, std):
    _check_sort_refusals(emu_lib, std)


@pytest.mark.gpu
def test_selftest_refusals_gpu(hip_lib, std):
    _check_sort_refusals(hip_lib, std)


# ---- the workgroup's 4-way partition ------------------------------------------------------------------------------------------------------

MX, MY = 700, 300
START, TAIL = 37, 29                                 # the span sits inside a larger buffer, at an offset that is no multiple of a wave


def _quadrant(keys):
    x, y = keys & 0xFFF, (keys >> 12) & 0xFFF
    left, top = x < MX, y < MY
    return np.where(left, np.where(top, 0, 2), np.where(top, 1, 3))


def _partition_keys(kind, c, rng):
    x = rng.integers(0, 2 * MX, c); y = rng.integers(0, 2 * MY, c)     # the lines halve the field, as a node's do
    if kind.startswith("all_in_"):                   # every key in one quadrant
        q = int(kind[-1])
        x = rng.integers(MX, 2 * MX, c) if q & 1 else rng.integers(0, MX, c)
        y = rng.integers(MY, 2 * MY, c) if q & 2 else rng.integers(0, MY, c)
    elif kind.startswith("none_in_"):                # one quadrant stays empty: its keys move across the vertical line
        q = int(kind[-1])
        inq = ((x >= MX) == bool(q & 1)) & ((y >= MY) == bool(q & 2))
        x = np.where(inq, x - MX if q & 1 else x + MX, x)
    elif kind == "on_the_lines":                     # keys exactly on mx / my and next to them
        x = MX + rng.integers(-1, 2, c); y = MY + rng.integers(-1, 2, c)
    return (x.astype(np.uint32) | (y.astype(np.uint32) << 12) | (rng.integers(0, 256, c).astype(np.uint32) << 24)).astype(np.uint32)


PARTITION_KINDS = tuple("all_in_%d" % q for q in range(4)) + tuple("none_in_%d" % q for q in range(4)) + ("on_the_lines", "random")


def _check_partition4(lib, threads):
    ex = _extractor(lib)
    lgnw = 2 if threads == 256 else 4
    rng = np.random.default_rng(77 + threads)
    for c in (1, 63, 64, 65, (64 << lgnw) - 1, (64 << lgnw) + 1, 1025, 5000):
        for kind in PARTITION_KINDS:
            total = START + c + TAIL
            src = rng.integers(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32)
            src[START:START + c] = _partition_keys(kind, c, rng)
            dst = rng.integers(0, 1 << 32, total, dtype=np.uint64).astype(np.uint32)
            span = src[START:START + c]
            q = _quadrant(span)
            if kind.startswith("all_in_"): assert (q == int(kind[-1])).all()
            if kind.startswith("none_in_"): assert not (q == int(kind[-1])).any() and (c < 64 or len(np.unique(q)) == 3)
            if kind == "on_the_lines" and c >= 63: assert len(np.unique(q)) == 4 and ((span & 0xFFF) == MX).any() and (((span >> 12) & 0xFFF) == MY).any()
            exp = span[np.argsort(q, kind="stable")]
            got, cnt = ex.debug_quadtree_partition4(src, dst, START, c, MX, MY, threads)
            where = "%s, span of %d, %d threads" % (kind, c, threads)
            assert cnt.tolist() == np.bincount(q, minlength=4).tolist(), where
            assert np.array_equal(got[START:START + c], exp), where
            assert np.array_equal(got[:START], dst[:START]) and np.array_equal(got[START + c:], dst[START + c:]), where + ": written outside the span"
    ex.close()


@pytest.mark.parametrize("threads", THREADS)
def test_partition4_emulated(emu_lib, threads):
    _check_partition4(emu_lib, threads)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
def test_partition4_gpu(hip_lib, threads):
    _check_partition4(hip_lib, threads)


# ---- the workgroup's 64-bit exclusive scan ------------------------------------------------------------------------------------------------

def _check_scan(lib, threads):
    ex = _extractor(lib)
    rng = np.random.default_rng(5 + threads)
    blocks = {
        "crosses_2^32": rng.integers(0, 1 << 30, threads, dtype=np.uint64),                                  # the total needs 38 .. 40 bits
        "three_fields": rng.integers(0, 4, threads, dtype=np.uint64) | rng.integers(0, 4, threads, dtype=np.uint64) << np.uint64(20) | np.uint64(1) << np.uint64(40),
        "zeros": np.zeros(threads, np.uint64),
        "last_thread_only": np.concatenate([np.zeros(threads - 1, np.uint64), np.array([(1 << 33) + 5], np.uint64)]),
        "carry_in_every_wave": np.full(threads, 0xFFFFFFFF, np.uint64),
    }
    for name, v in blocks.items():
        inc = np.cumsum(v, dtype=np.uint64)
        if name in ("crosses_2^32", "carry_in_every_wave"): assert int(inc[-1]) > 1 << 32
        got, tot = ex.debug_quadtree_scan(v)
        assert np.array_equal(got, inc - v) and tot == int(inc[-1]), (name, threads)
    ex.close()


@pytest.mark.parametrize("threads", THREADS)
def test_scan_emulated(emu_lib, threads):
    _check_scan(emu_lib, threads)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", THREADS)
def test_scan_gpu(hip_lib, threads):
    _check_scan(hip_lib, threads)
