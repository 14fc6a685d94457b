"""No GPU: the parameters of the fp16 traversal (index-time gpu_rows, query-time gpu_rows / gpu_rerank) through the C
ABI on indexes whose upload is deferred, and the packing header (scale choice, rounding) in a stand-alone program built
with the host sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests.gpuutil import FLOAT_SPACES, make_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = np.random.default_rng(3).standard_normal((60, 12)).astype(np.float32)


def refused(fn, *needles):
    with pytest.raises(nz.NmslibError) as ei:
        fn()
    assert ei.value.code == 2, ei.value                      # NMSLIB_ERROR_INVALID_ARGUMENT
    for s in needles:
        assert s in str(ei.value), ei.value


@pytest.mark.parametrize("space", FLOAT_SPACES)
def test_gpu_rows_is_accepted_for_the_float_spaces_and_round_trips(space):
    idx = make_index(space, "hnsw", X, M=6, efConstruction=20, indexThreadQty=1, gpu_defer=1, gpu_rows="f16")
    idx.setQueryTimeParams(efSearch=40, gpu_rows="f32")
    idx.setQueryTimeParams(efSearch=40, gpu_rows="f16", gpu_rerank=25)
    idx.setQueryTimeParams(efSearch=40)                          # the extensions stay as set
    idx.setQueryTimeParams(gpu_rerank=1)                         # (clamped to k at query time)
    idx.close()
    idx = make_index(space, "hnsw", X, M=6, efConstruction=20, indexThreadQty=1, gpu_defer=1, gpu_rows="f32")
    idx.setQueryTimeParams(gpu_rows="f16")
    idx.close()


def test_bad_values_are_refused_with_a_reason():
    refused(lambda: make_index("l2", "hnsw", X, gpu_defer=1, gpu_rows="bf16"), "gpu_rows", "f32 or f16", "bf16")
    idx = make_index("l2", "hnsw", X, M=6, efConstruction=20, indexThreadQty=1, gpu_defer=1)
    refused(lambda: idx.setQueryTimeParams(gpu_rows="bf16"), "gpu_rows", "f32 or f16")
    refused(lambda: idx.setQueryTimeParams(gpu_rerank=0), "gpu_rerank", "at least 1")
    refused(lambda: idx.setQueryTimeParams(gpu_rerank=-3), "gpu_rerank")
    idx.setQueryTimeParams(gpu_rows="f16", gpu_rerank=10)        # the index still takes good values
    idx.close()


def test_f16_is_refused_where_there_are_no_float_rows():
    U = np.random.default_rng(4).integers(0, 255, (40, 128)).astype(np.uint8)
    refused(lambda: make_index("l2sqr_sift", "hnsw", U, gpu_defer=1, gpu_rows="f16"), "l2sqr_sift", "uint8")
    idx = make_index("l2sqr_sift", "hnsw", U, M=6, efConstruction=20, indexThreadQty=1, gpu_defer=1, gpu_rows="f32")
    refused(lambda: idx.setQueryTimeParams(gpu_rows="f16"), "l2sqr_sift")
    idx.close()
    words = ["kitten", "sitting", "mitten", "fitting", "bitten", "knitting", "written", "smitten"]
    s = nz.Index("leven", "hnsw", data_type="ObjectAsString", dist_type="Int")
    s.addStringBatch(words)
    refused(lambda: s.buildIndex(M=4, efConstruction=10, indexThreadQty=1, gpu_defer=1, gpu_rows="f16"), "string", "float rows")
    s.close()
    s = nz.Index("leven", "hnsw", data_type="ObjectAsString", dist_type="Int")
    s.addStringBatch(words)
    s.buildIndex(M=4, efConstruction=10, indexThreadQty=1, gpu_defer=1)
    refused(lambda: s.setQueryTimeParams(gpu_rows="f16"), "string")
    s.close()


@pytest.mark.parametrize("method", ["brute_force", "seq_search"])
def test_the_exact_scan_keeps_refusing_it_as_an_unknown_parameter(method):
    with pytest.raises(nz.NmslibError) as ei:
        make_index("l2", method, X, gpu_defer=1, gpu_rows="f16")
    assert ei.value.code == 8 and "Unknown parameters" in str(ei.value), ei.value


def test_packing_header_standalone_under_host_sanitizers(tmp_path):
    """tests/f16_pack_check.cpp includes csrc/f16_pack.hpp alone (no HIP): rows spanning 2^-30 .. 2^30 get a power-of-two
    scale, no packed value is inf or NaN, the largest lands in [2^14, 2^15) (checked by the program); every rounding equals
    numpy's float16 on the scaled value (checked here, edge values included)."""
    exe, out = str(tmp_path / "f16_pack_check"), str(tmp_path / "f16.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "f16_pack_check.cpp"), "-o", exe])
    run = subprocess.run([exe, out], capture_output=True, text=True)
    assert run.returncode == 0 and "f16 pack ok" in run.stdout, run.stdout + run.stderr
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw[:4], np.uint32)[0])
    vals = np.frombuffer(raw[4:4 + 4 * n], np.float32)
    bits = np.frombuffer(raw[4 + 4 * n:], np.uint16)
    assert n > 2000 and len(bits) == n
    with np.errstate(over="ignore"):
        want = vals.astype(np.float16).view(np.uint16)
    np.testing.assert_array_equal(bits, want)
    assert ((bits & 0x7C00) == 0).sum() > 100                    # the subnormal branch was exercised
