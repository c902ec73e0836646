"""CPU only: the eight-wave hidden-layer backward (k_bwd_dx_dw8, mlp.hip) must compile, with the library's own flags, to at most
256 registers per wave (VGPR + AGPR) with no scratch, i.e. two waves per SIMD -- the point of running the owner and the
weight-gradient parts on waves of their own.  Reads hipcc's kernel-resource-usage remarks; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

from harl_amd import _build


def _resources():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(_build.CSRC, "mlp.hip"), "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"] + _build.EXTRA_FLAGS.get("mlp.hip", [])
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows, cur = {}, None
    for ln in err.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"remark:\s+(\w[\w \[\]/]*?): (\d+)", ln)
        if m and cur:
            rows[cur][m.group(1).strip()] = int(m.group(2))
    return rows


@pytest.fixture(scope="module")
def resources():
    return _resources()


def test_split_wave_kernel_occupancy_two(resources):
    # the four instantiations <KT, FILL>: Itanium names _Z12k_bwd_dx_dw8ILi<KT>ELb<FILL>E...
    found = {k: v for k, v in resources.items() if k.startswith("_Z12k_bwd_dx_dw8I")}
    assert len(found) == 4, sorted(resources)
    for name, r in found.items():
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 256, (name, r)
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
        assert r.get("VGPRs Spill", 0) == 0, (name, r)
        assert r.get("Occupancy [waves/SIMD]", 0) >= 2, (name, r)
