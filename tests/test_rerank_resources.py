"""No GPU: what the compiler gives every instantiation of bf_rerank_f32_list_kernel (hipcc cross-compiles).

The list re-rank of the exact f32 scan launches one workgroup of four waves per query; how many of them a CU holds at
once decides whether a batch of 1024 queries runs in one round of resident workgroups or in two (DESIGN.md 4.1b
"Residency").  The instantiations for rows of up to 128 dimensions must fit 128 VGPRs without scratch (occupancy 4 or
more), and the LDS of every instantiation at the C2 plan must let four workgroups share the 160 KB of a CU.  The test
reads the compiler's kernel-info blocks only."""
import math
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_PER_CU = 160 * 1024
BF_BN = 64


def _next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def lds_rerank_c2(n=1_000_000, nq=1024, k=10):
    """bf_f32_fast_plan's dynamic LDS of the list re-rank (rows of up to 128 dimensions), recomputed from its formula."""
    qg = 2 if nq >= 1024 else 1
    tq = 256 * qg
    nqt = (nq + tq - 1) // tq
    stride = 16
    kp = k + max(4, k // 8)
    kf = kp / stride
    r = int(1.6 * kf + 3.0 * math.sqrt(kf) + 3.0 + 0.999)
    rcap = 4 * r + 32
    tiles_all = (n + BF_BN - 1) // BF_BN
    ns = min((256 + nqt - 1) // nqt, tiles_all // 16, 256)
    ns = max((ns + 7) // 8 * 8, 8)
    while (tiles_all + ns - 1) // ns > 32768:
        ns += 8
    mean_half = rcap * stride / (2.0 * ns)
    caph = 8
    while caph < 3.0 * mean_half + 8.0:
        caph <<= 1
    p2max = _next_pow2(int(2.5 * rcap * stride) + 64)
    if p2max > 2 * ns * caph:
        p2max = _next_pow2(2 * ns * caph)
    return p2max * 8 + (2 * ns + 1) * 4 + 16


@pytest.fixture(scope="module")
def kernel_info(tmp_path_factory):
    """{(space, centred, long rows): {NumVgprs, ScratchSize, Occupancy, LDSByteSize, ...}} of every instantiation."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "nmslib_zig_amd", "csrc", "kernels", "bf_kernels.hip")
    asm = str(tmp_path_factory.mktemp("rerank_asm") / "bf.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-pass-failed", "-mllvm",
                           "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only", src, "-o", asm],
                          stderr=subprocess.DEVNULL)
    info, cur = {}, None
    for line in open(asm):
        m = re.match(r"^_ZN6gfxknn\d+bf_rerank_f32_list_kernelILi(\d+)ELb([01])ELb([01])EEEv\w+:", line)
        if m:
            cur = info.setdefault((int(m.group(1)), m.group(2) == "1", m.group(3) == "1"), {})
            continue
        if cur is not None:
            m = re.match(r"^; (\w+): (\d+)", line)
            if m:
                cur[m.group(1)] = int(m.group(2))
                if m.group(1) == "Occupancy":
                    cur = None
    return info


def test_every_instantiation_is_there(kernel_info):
    """l2 (0), negdotprod (5), cosinesimil (3) and angulardist (4), the last two also centred; short and long rows."""
    want = {(s, c, lng) for s, c in ((0, False), (5, False), (3, False), (3, True), (4, False), (4, True)) for lng in (False, True)}
    assert set(kernel_info) == want, sorted(kernel_info)


def test_short_row_instantiations_fit_four_waves_per_simd(kernel_info):
    short = {key: v for key, v in kernel_info.items() if not key[2]}
    assert len(short) == 6
    for key, v in short.items():
        print(key, v)
        assert max(v["NumVgprs"], v.get("TotalNumVgprs", 0)) <= 128, (key, v)
        assert v["ScratchSize"] == 0, (key, v)
        assert v["Occupancy"] >= 4, (key, v)


def test_four_workgroups_share_a_cu_lds(kernel_info):
    dyn = lds_rerank_c2()
    assert dyn == 4096 * 8 + 257 * 4 + 16
    for key, v in kernel_info.items():
        assert 4 * (v["LDSByteSize"] + dyn) <= LDS_PER_CU, (key, v, dyn)
