"""The DEVICE build of the bit-exact function models, swept over their domains: glibc_cosf / glibc_sinf (csrc/glibc_sincosf_model.h), glibc_logf_model<false>
(glibc_logf_model.h), glibc_tanf_model (glibc_tanf_model.h), glibc_atanf_model / glibc_atan2f_model (glibc_atan2f_model.h), fast_atan2_deg and the steering
triple of k_orient_brief (csrc/k_describe.hip), evaluated by the shipped library (orbx_debug_model_eval -> k_model_selftest, built by the ordinary Makefile rule
with the ordinary flags) and compared bit for bit - NaN with NaN counts as equal, nothing else does - with the LIVE libm, with cv::fastAtan2 as
oracle/orb_primitives.h restates it, and with both composed (tests/cpp/libm_sweep.cpp, up to 16 threads).

On the GPU every float of a one-argument domain is compared: [-6.5, 6.5] for cosf / sinf, every positive finite float (subnormals included) for logf, [0, 8] for
tanf, all 2^32 bit patterns for atanf.  atan2f, fastAtan2 and the steering take explicit pairs (below).  Every case asserts the number of elements it compared
against the formula of its domain, so a thinned sweep fails.  The emulated cases run the same code path on the CPU build with every 4099th bit pattern, the
first and last 4096 patterns of every range, the special-value cross product and 2^16 pairs of every other kind.

What this does NOT show: k_model_selftest is an instantiation of its own of the inline functions, not the copy inlined into k_orient_brief, k_frustum or
k_kb8_stereo.  Without fast-math flags IEEE fixes the arithmetic of both, so they agree; the one place where the composition matters - angle, angle * factorPI,
cos, sin - is a helper (steer_from_moments) that k_orient_brief and op 7 both call.  The kernel's code object is not inspected.

A mismatch is reported with the input bits, the result bits of the device build, of the host build of the same header (host_model) and of the host's expectation,
and the count of the chunk; the sweep stops at the first chunk that has one.  The host build reproduces it on a CPU: there is no need to run a sweep twice."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

from orb_slam3_detailed_comments_amd import _lib
from orb_slam3_detailed_comments_amd.extractor import ORBextractor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam3_detailed_comments_amd", "csrc")
THREADS = min(16, len(os.sched_getaffinity(0)))
CHUNK = 1 << 26                                                  # elements per call: the limit of orbx_debug_model_eval, and 256 MB of results
COSF, SINF, LOGF, TANF, ATANF, ATAN2F, FASTATAN2, STEER = range(8)
NAMES = ["cosf", "sinf", "logf", "tanf", "atanf", "atan2f", "fastAtan2", "steering"]


def _bits(x):
    return int(np.float32(x).view(np.uint32))


# the one-argument domains as (first bit pattern, count) ranges
B65, B8 = _bits(6.5), _bits(8.0)
RANGES = {
    COSF: [(0, B65 + 1), (0x80000000, B65 + 1)],                 # [0, 6.5] and [-0, -6.5]
    SINF: [(0, B65 + 1), (0x80000000, B65 + 1)],
    LOGF: [(1, 0x7f7fffff)],                                     # smallest subnormal .. FLT_MAX
    TANF: [(0, B8 + 1)],
}
assert B65 + 1 == 1087373313 and B8 + 1 == 1090519041 and RANGES[LOGF][0][1] == 2139095039


@functools.lru_cache(maxsize=None)
def comparer():
    td = tempfile.mkdtemp(prefix="libm_sweep_")
    so = os.path.join(td, "libm_sweep.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "libm_sweep.cpp"), "-o", so, "-lpthread"],
                   check=True)
    L = C.CDLL(so)
    L.sweep_compare.restype = C.c_longlong
    L.sweep_compare.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]
    for f in (L.host_model, L.host_expect):
        f.restype = C.c_int; f.argtypes = [C.c_int, C.c_float, C.c_float, C.c_void_p]
    L.fast_atan2_many.restype = None
    L.fast_atan2_many.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int]
    return L


def _ptr(x):
    return None if x is None else x.ctypes.data


def evaluate(ex, op, start_bits, a, b, n, out):
    """out[: n] (out[: 3 n] for the steering) = the library's results"""
    assert out.dtype == np.float32 and out.flags.c_contiguous and len(out) >= (3 * n if op == STEER else n)
    ex._lib.check(ex._lib.L.orbx_debug_model_eval(ex._h, op, start_bits, _ptr(a), _ptr(b), n, out.ctypes.data))


def compare(op, start_bits, a, b, n, out):
    """(number of mismatches, index of the first) of out against the host's expectation"""
    first = C.c_longlong(-2)
    bad = comparer().sweep_compare(op, start_bits, _ptr(a), _ptr(b), n, out.ctypes.data, THREADS, C.byref(first))
    assert bad >= 0, "sweep_compare refused its arguments"
    return int(bad), int(first.value)


def _same(p, q):
    p, q = np.asarray(p, np.float32), np.asarray(q, np.float32)
    return len(p) == len(q) and bool(np.all((p.view(np.uint32) == q.view(np.uint32)) | (np.isnan(p) & np.isnan(q))))


def _describe(op, start_bits, a, b, n, out, bad, first):
    L = comparer()
    x = np.float32(a[first]) if a is not None else np.array([(start_bits + first) & 0xFFFFFFFF], np.uint32).view(np.float32)[0]
    y = np.float32(b[first]) if b is not None else np.float32(0)
    dev = np.array([out[first + k * n] for k in range(3 if op == STEER else 1)], np.float32)
    model, want = np.zeros(3, np.float32), np.zeros(3, np.float32)
    nm = L.host_model(op, float(x), float(y), model.ctypes.data); nw = L.host_expect(op, float(x), float(y), want.ctypes.data)
    hexs = lambda v: " ".join("%08x" % int(u) for u in np.asarray(v, np.float32).view(np.uint32))
    if nm == 0:
        verdict = "no host build of this function (the emulated case is its host build)"
    elif _same(dev, model[:nm]):
        verdict = "device == host build != expectation: the header is wrong for this input, or this machine's libm is not the glibc the model was written for"
    elif _same(model[:nm], want[:nw]):
        verdict = "host build == expectation != device: the device compiler's build of the header differs (contraction, division, denormals, conversions)"
    else:
        verdict = "device, host build and expectation all differ"
    return ("%s: %d mismatches in this chunk of %d; first at index %d: input bits %08x %08x, device %s, host build %s, expectation %s - %s"
            % (NAMES[op], bad, n, first, int(x.view(np.uint32)), int(y.view(np.uint32)), hexs(dev), hexs(model[:nm]) if nm else "-", hexs(want[:nw]), verdict))


def check_chunk(ex, op, start_bits, a, b, n, out):
    evaluate(ex, op, start_bits, a, b, n, out)
    bad, first = compare(op, start_bits, a, b, n, out)
    if bad:
        pytest.fail(_describe(op, start_bits, a, b, n, out, bad, first))
    return n


def walk_ranges(ex, op, ranges, out):
    """every bit pattern of the ranges, in chunks of at most CHUNK; returns the number of elements compared"""
    covered = 0
    for start, count in ranges:
        for off in range(0, count, CHUNK):
            covered += check_chunk(ex, op, (start + off) & 0xFFFFFFFF, None, None, min(CHUNK, count - off), out)
    return covered


def walk_pairs(ex, op, blocks, out):
    """blocks: iterable of (a, b) float32 arrays; returns the number of pairs compared"""
    step = len(out) // 3 if op == STEER else min(len(out), CHUNK)
    covered = 0
    for a, b in blocks:
        a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
        assert a.shape == b.shape and a.ndim == 1
        for off in range(0, len(a), step):
            covered += check_chunk(ex, op, 0, a[off:off + step], b[off:off + step], len(a[off:off + step]), out)
    return covered


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# atan2f pairs (first operand y, second x)
F32 = np.finfo(np.float32)
SPECIALS = np.array([s * v for v in (0.0, float(F32.smallest_subnormal), float(np.array([0x007fffff], np.uint32).view(np.float32)[0]), float(F32.tiny), 1.0,
                                     float(F32.max), np.inf) for s in (1.0, -1.0)] + [np.nan], np.float32)
K_POW2 = np.arange(-70, 71)                                      # y = x * 2^k: across both cut-offs of e_atan2f.c (|k| > 60)


def _random_floats(rng, n, emin, emax):
    """random signs and mantissas, exponents uniform in [emin, emax]"""
    return np.ldexp((rng.random(n, np.float32) + np.float32(1)) * rng.choice(np.array([-1, 1], np.float32), n), rng.integers(emin, emax + 1, n).astype(np.int32)).astype(np.float32)


def _random_bits(rng, n):
    return np.frombuffer(rng.bytes(4 * n), np.uint32).view(np.float32)


def atan2_special_pairs():
    y, x = np.meshgrid(SPECIALS, SPECIALS, indexing="ij")
    return y.ravel().copy(), x.ravel().copy()


def atan2_pow2_pairs(rng, nx):
    """y = x * 2^k for k in [-70, 70]; x with exponents in [-60, 60], so that y also overflows to inf and runs into the subnormals"""
    x = _random_floats(rng, nx, -60, 60)
    with np.errstate(over="ignore", under="ignore"):
        y = np.ldexp(x[:, None], K_POW2[None, :].astype(np.int32)).astype(np.float32)
    return y.ravel(), np.repeat(x, len(K_POW2))


def atan2_x_one_pairs(rng, n):
    """the shortcut x == 1.0f -> atanf(y)"""
    return _random_bits(rng, n), np.ones(n, np.float32)


def atan2_subnormal_quotient_pairs(rng, n):
    """y / x in the subnormal range (or rounding to zero) with x > 0 or x < 0: the quotient itself is a denormal the device must keep"""
    x = _random_floats(rng, n, 0, 100)
    e = np.frexp(np.abs(x))[1].astype(np.int32)
    with np.errstate(under="ignore"):
        y = np.ldexp(rng.random(n, np.float32) + np.float32(1), (e + rng.integers(-151, -126, n)).astype(np.int32)).astype(np.float32)
    return y * rng.choice(np.array([-1, 1], np.float32), n), x


def atan2_kb8_pairs(rng, npoints):
    """the two calls of KannalaBrandt8::project on points p uniform in [-10, 10]^3: atan2f(sqrtf(px^2 + py^2), pz) and atan2f(py, px); 2 * npoints pairs"""
    p = rng.random((3, npoints), np.float32) * np.float32(20) - np.float32(10)
    r = np.sqrt(p[0] * p[0] + p[1] * p[1])                       # float32 throughout, as the reference computes it
    return np.concatenate([r, p[1]]), np.concatenate([p[2], p[0]])


N_ATAN2_GPU = 1 << 28
N_ATAN2_STRUCTURED = len(SPECIALS) ** 2 + (1 << 16) * len(K_POW2) + (1 << 24) + (1 << 16)       # all but the Kannala-Brandt pairs and the random fill


def atan2_block_gpu(k):
    """2^28 pairs in four blocks of 2^26, built one at a time: the structured kinds filled up with random bit patterns, the Kannala-Brandt pairs, two
    blocks of random bit patterns"""
    rng = np.random.default_rng([20261019, k])
    if k == 0:
        kinds = [atan2_special_pairs(), atan2_pow2_pairs(rng, 1 << 16), atan2_x_one_pairs(rng, 1 << 24), atan2_subnormal_quotient_pairs(rng, 1 << 16)]
        assert sum(len(q[0]) for q in kinds) == N_ATAN2_STRUCTURED and len(SPECIALS) == 15
        fill = CHUNK - N_ATAN2_STRUCTURED
        return np.concatenate([q[0] for q in kinds] + [_random_bits(rng, fill)]), np.concatenate([q[1] for q in kinds] + [_random_bits(rng, fill)])
    if k == 1:
        return atan2_kb8_pairs(rng, 1 << 25)
    return _random_bits(rng, CHUNK), _random_bits(rng, CHUNK)


def atan2_blocks_emulated():
    rng = np.random.default_rng(20261020)
    kinds = [atan2_special_pairs(), atan2_pow2_pairs(rng, (1 << 16) // len(K_POW2) + 1), atan2_x_one_pairs(rng, 1 << 16), atan2_subnormal_quotient_pairs(rng, 1 << 16),
             atan2_kb8_pairs(rng, 1 << 15), (_random_bits(rng, 1 << 16), _random_bits(rng, 1 << 16))]
    yield np.concatenate([k[0] for k in kinds]), np.concatenate([k[1] for k in kinds])


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# fastAtan2 and steering pairs (first operand m01, second m10): integer-valued moments
HALF_PATCH, GRID = 15, 2048
AXIS_ANGLES = (0.0, 90.0, 180.0, 270.0, 360.0)


def oracle_umax():
    """the circular patch as the oracle builds it (oracle/orb_oracle.cpp, reference src/ORBextractor.cc:542-570)"""
    vmax = int(np.floor(HALF_PATCH * np.sqrt(2.0) / 2 + 1)); vmin = int(np.ceil(HALF_PATCH * np.sqrt(2.0) / 2))
    um = [0] * (HALF_PATCH + 1)
    for v in range(vmax + 1):
        um[v] = int(np.rint(np.sqrt(float(HALF_PATCH * HALF_PATCH - v * v))))        # rint: round half to even, as cvRound
    v0 = 0
    for v in range(HALF_PATCH, vmin - 1, -1):
        while um[v0] == um[v0 + 1]:
            v0 += 1
        um[v] = v0
        v0 += 1
    return um


def moment_bound(ex):
    """the largest |m10|, |m01| of IC_Angle: every pixel of the patch at 255, 255 * sum(|u|)"""
    um = oracle_umax()
    assert list(ex.umax()[:HALF_PATCH + 1]) == um, "the library's patch is not the oracle's"
    bound = 255 * sum(sum(abs(u) for u in range(-um[abs(v)], um[abs(v)] + 1)) for v in range(-HALF_PATCH, HALF_PATCH + 1))
    assert bound == 1248480 and GRID < bound < 1 << 24             # 4896 * 255; the moments are exact in fp32
    return bound


def moment_grid():
    """every pair with |m01|, |m10| <= 2048: (0, 0), both axes, both diagonals (where ax >= ay picks the branch)"""
    v = np.arange(-GRID, GRID + 1, dtype=np.float32)
    m01, m10 = np.meshgrid(v, v, indexing="ij")
    return m01.ravel(), m10.ravel()


def moment_near_axis_pairs(bound):
    """|small| <= 8 against the largest moments, both orders and all signs: the angles closest to the axes that integer moments reach"""
    big = np.array([bound, bound - 1, bound // 2, 1 << 20, 1 << 19, 999999, GRID + 1], np.float32)
    small = np.arange(-8, 9, dtype=np.float32)
    s, g = (x.ravel() for x in np.meshgrid(small, np.concatenate([big, -big]), indexing="ij"))
    return np.concatenate([s, g]), np.concatenate([g, s])


def moment_random_pairs(rng, n, bound):
    return rng.integers(-bound, bound + 1, n).astype(np.float32), rng.integers(-bound, bound + 1, n).astype(np.float32)


def axis_neighbours(blocks):
    """the pairs of `blocks` whose fastAtan2 angle lies within 2 ulp of 0, 90, 180, 270 or 360 degrees (host scan): angle * factorPI is then at both ends
    of the range-reduction branches of the cos / sin model.  Returns (m01, m10, the set of axis angles that were reached)."""
    L = comparer()
    targets = np.array([_bits(t) for t in AXIS_ANGLES], np.int64)
    sel_a, sel_b, hit = [], [], set()
    for a, b in blocks:
        a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
        ang = np.empty(len(a), np.float32)
        L.fast_atan2_many(a.ctypes.data, b.ctypes.data, len(a), ang.ctypes.data, THREADS)
        ab = ang.view(np.uint32).astype(np.int64)
        near = np.zeros(len(a), bool)
        for t, tb in zip(AXIS_ANGLES, targets):
            m = np.abs(ab - tb) <= 2
            if m.any():
                hit.add(t)
            near |= m
        sel_a.append(a[near]); sel_b.append(b[near])
    return np.concatenate(sel_a), np.concatenate(sel_b), hit


def moment_blocks(ex, steering, nrandom, grid_sample=None):
    """the blocks of a fastAtan2 / steering case and their expected pair count.  grid_sample: the emulated cases take that many random pairs of the grid
    instead of all of it (the scan for the axis neighbours always reads the whole grid)."""
    bound = moment_bound(ex)
    rng = np.random.default_rng(20261021)
    grid, near, rnd = moment_grid(), moment_near_axis_pairs(bound), moment_random_pairs(rng, nrandom, bound)
    assert len(grid[0]) == (2 * GRID + 1) ** 2 and len(near[0]) == 2 * 17 * 14
    blocks = [near, rnd]
    if grid_sample is None:
        blocks.append(grid)
    else:
        pick = rng.integers(0, len(grid[0]), grid_sample)
        blocks.append((grid[0][pick], grid[1][pick]))
    expected = sum(len(b[0]) for b in blocks)
    if steering:
        a, b, hit = axis_neighbours([grid, near, rnd])
        assert hit == set(AXIS_ANGLES) and len(a) >= 4 * GRID, "the scan must reach all five axis angles (found %s, %d pairs)" % (sorted(hit), len(a))
        blocks.insert(0, (a, b)); expected += len(a)
    return blocks, expected


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# GPU: whole domains
@pytest.fixture(scope="module")
def gpu_ex(hip_lib):
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=hip_lib)
    yield ex
    ex.close()


@pytest.fixture(scope="module")
def gpu_out():
    return np.empty(CHUNK, np.float32)                           # 256 MB, shared by every case


GPU_RANGE_CASES = [("cosf", COSF, RANGES[COSF]), ("sinf", SINF, RANGES[SINF]), ("logf", LOGF, RANGES[LOGF]), ("tanf", TANF, RANGES[TANF]),
                   ("atanf", ATANF, [(0, 1 << 32)])]                                                                  # all 2^32 bit patterns, NaNs included


@pytest.mark.gpu
@pytest.mark.parametrize("name,op,ranges", GPU_RANGE_CASES, ids=[c[0] for c in GPU_RANGE_CASES])
def test_whole_domain_gpu(gpu_ex, gpu_out, name, op, ranges):
    expected = {"cosf": 2 * 1087373313, "sinf": 2 * 1087373313, "logf": 2139095039, "tanf": 1090519041, "atanf": 4294967296}[name]
    assert walk_ranges(gpu_ex, op, ranges, gpu_out) == expected


@pytest.mark.gpu
def test_atan2f_pairs_gpu(gpu_ex, gpu_out):
    assert walk_pairs(gpu_ex, ATAN2F, (atan2_block_gpu(k) for k in range(4)), gpu_out) == N_ATAN2_GPU == 4 * CHUNK


@pytest.mark.gpu
@pytest.mark.parametrize("op", [FASTATAN2, STEER], ids=["fastAtan2", "steering"])
def test_moment_pairs_gpu(gpu_ex, gpu_out, op):
    blocks, expected = moment_blocks(gpu_ex, op == STEER, 1 << 24)
    base = (2 * GRID + 1) ** 2 + (1 << 24) + 2 * 17 * 14          # the whole grid, the random pairs, the constructed near-axis pairs
    assert expected == base if op == FASTATAN2 else expected >= base + 4 * GRID
    assert walk_pairs(gpu_ex, op, blocks, gpu_out) == expected


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# emulator: the same code path on the CPU build
STRIDE, EDGE = 4099, 4096


@pytest.fixture(scope="module")
def emu_ex(emu_lib):
    ex = ORBextractor(500, 1.2, 8, 20, 7, lib=emu_lib)
    yield ex
    ex.close()


def _check_thinned(ex, op, ranges):
    out = np.empty(1 << 21, np.float32)
    covered = 0
    for start, count in ranges:
        assert count >= 2 * EDGE
        covered += check_chunk(ex, op, start, None, None, EDGE, out)                                          # the first and the last 4096 patterns, by start_bits
        covered += check_chunk(ex, op, (start + count - EDGE) & 0xFFFFFFFF, None, None, EDGE, out)
        a = (np.arange(start, start + count, STRIDE, dtype=np.uint64) & 0xFFFFFFFF).astype(np.uint32).view(np.float32)    # every 4099th, as operands
        covered += walk_pairs(ex, op, [(a, np.zeros_like(a))], out)
        assert len(a) == -(-count // STRIDE)
    return covered


@pytest.mark.parametrize("op", [COSF, SINF, LOGF, TANF, ATANF], ids=NAMES[:5])
def test_thinned_domain_emulated(emu_ex, op):
    ranges = RANGES.get(op) or [(0, 1 << 31), (0x80000000, 1 << 31)]     # atanf: the edges of both signs (+-0, +-NaN with every bit set)
    assert _check_thinned(emu_ex, op, ranges) == sum(2 * EDGE + -(-count // STRIDE) for _, count in ranges)


def test_atan2f_pairs_emulated(emu_ex):
    out = np.empty(1 << 21, np.float32)
    n = walk_pairs(emu_ex, ATAN2F, atan2_blocks_emulated(), out)
    assert n == len(SPECIALS) ** 2 + ((1 << 16) // len(K_POW2) + 1) * len(K_POW2) + 4 * (1 << 16)


@pytest.mark.parametrize("op", [FASTATAN2, STEER], ids=["fastAtan2", "steering"])
def test_moment_pairs_emulated(emu_ex, op):
    out = np.empty(3 << 19, np.float32)
    blocks, expected = moment_blocks(emu_ex, op == STEER, 1 << 16, grid_sample=1 << 16)
    assert walk_pairs(emu_ex, op, blocks, out) == expected


def test_comparer_reports_a_flipped_bit(emu_ex):
    """The comparer can fail: one low bit flipped in a chunk of correct results (a host array; nothing runs on a device) is reported as one mismatch at that index,
    for a range sweep, a pair sweep and in each of the three planes of the steering; a NaN with another payload is still equal to a NaN, a number is not."""
    n = 4096
    out = np.empty(3 * n, np.float32)
    start = _bits(1.0) - 100
    evaluate(emu_ex, ATANF, start, None, None, n, out)
    assert compare(ATANF, start, None, None, n, out) == (0, -1)
    out.view(np.uint32)[1234] ^= 1
    assert compare(ATANF, start, None, None, n, out) == (1, 1234)
    out.view(np.uint32)[4000] ^= 1
    assert compare(ATANF, start, None, None, n, out) == (2, 1234)
    rng = np.random.default_rng(3)
    y, x = _random_floats(rng, n, -20, 20), _random_floats(rng, n, -20, 20)
    evaluate(emu_ex, ATAN2F, 0, y, x, n, out)
    assert compare(ATAN2F, 0, y, x, n, out) == (0, -1)
    out.view(np.uint32)[n - 1] ^= 1
    assert compare(ATAN2F, 0, y, x, n, out) == (1, n - 1)
    m01, m10 = moment_random_pairs(rng, n, 100000)
    for plane, index in ((0, 7), (1, 2048), (2, 0)):
        evaluate(emu_ex, STEER, 0, m01, m10, n, out)
        assert compare(STEER, 0, m01, m10, n, out) == (0, -1)
        out.view(np.uint32)[plane * n + index] ^= 1
        assert compare(STEER, 0, m01, m10, n, out) == (1, index)
    nan_in = np.full(n, np.nan, np.float32); res = np.zeros(n, np.float32)
    res.view(np.uint32)[:] = 0xFFC00123                                                          # NaNs of another sign and payload
    assert compare(ATANF, 0, nan_in, np.zeros(n, np.float32), n, res) == (0, -1)
    res[17] = 1.5
    assert compare(ATANF, 0, nan_in, np.zeros(n, np.float32), n, res) == (1, 17)


def test_model_eval_refuses_bad_arguments(emu_ex):
    f = emu_ex._lib.L.orbx_debug_model_eval
    out = np.full(64, 7.0, np.float32); a = np.ones(16, np.float32); b = np.ones(16, np.float32)
    o, pa, pb = out.ctypes.data, a.ctypes.data, b.ctypes.data
    h = emu_ex._h
    refused = [(h, 0, 0, None, None, 0, o), (h, 0, 0, None, None, -1, o), (h, 0, 0, None, None, (1 << 26) + 1, o),        # n
               (h, 8, 0, pa, pb, 16, o), (h, -1, 0, pa, pb, 16, o),                                                       # op
               (h, 0, 0, None, None, 16, None), (h, 5, 0, pa, pb, 16, None),                                              # out
               (None, 0, 0, None, None, 16, o)]                                                                           # handle
    refused += [(h, op, 0, pa, None, 16, o) for op in (5, 6, 7)] + [(h, op, 0, None, pb, 16, o) for op in (5, 6, 7)] + [(h, op, 0, None, None, 16, o) for op in (5, 6, 7)]
    for args in refused:
        assert f(*args) == _lib.ORBX_E_ARG, args
    assert (out == 7.0).all(), "a refused call must not launch"
    assert f(h, 4, 0, pa, None, 16, o) == 0 and f(h, 0, 0, None, None, 16, o) == 0 and f(h, 7, 0, pa, pb, 16, o) == 0     # and the accepted forms
    assert not (out[:48] == 7.0).any() and (out[48:] == 7.0).all()
