"""CPU only: the fused hidden-layer backward without filler slots, which harl_mlp_bwd_dx_dw launches by default at two waves per
SIMD (fill = 1; profiles/r10_update_trims.md).  The no-filler instantiations of k_bwd_dx_dw8 must still compile, with the
library's own flags, to at most 256 registers per wave (VGPR + AGPR) with no scratch -- two waves per SIMD is what makes the
fillers unnecessary -- and HARL_BWD_FUSED must reach the launch as documented.  No GPU needed."""
import pytest

from tests.test_bwd_split_waves_res_cpu import _resources
from tests.test_hybrid_cpu import _runner, _train
from tests.test_multidiscrete_cpu import stub_kernels  # noqa: F401  (fixture)


@pytest.fixture(scope="module")
def resources():
    return _resources()


def test_no_filler_instantiations_keep_two_waves_per_simd(resources):
    # Itanium names _Z12k_bwd_dx_dw8ILi<KT>ELb<FILL>E...: FILL = false for KT = 0 (dz_prev stored) and KT = 1 (fused dW_1')
    found = {k: v for k, v in resources.items() if k.startswith("_Z12k_bwd_dx_dw8ILi") and "ELb0E" in k[:28]}
    assert len(found) == 2, sorted(k for k in resources if "k_bwd_dx_dw8" in k)
    for name, r in found.items():
        assert r["VGPRs"] + r.get("AGPRs", 0) <= 256, (name, r)
        assert r.get("ScratchSize [bytes/lane]", 0) == 0, (name, r)
        assert r.get("VGPRs Spill", 0) == 0, (name, r)
        assert r.get("Occupancy [waves/SIMD]", 0) >= 2, (name, r)


def test_fill_argument_follows_the_switch(stub_kernels, monkeypatch):  # noqa: F811
    """fill (argument 14 of harl_mlp_bwd_dx_dw): 1 = the library's choice for "1" and "auto", 0 for "nofill", 2 for "fill"."""
    for mode, want in (("1", 1), ("nofill", 0), ("fill", 2)):
        monkeypatch.setenv("HARL_BWD_FUSED", mode)
        n = _train(_runner([128, 128]), stub_kernels)
        assert n["harl_mlp_bwd_dx_dw"] > 0
        assert {c[14] for c in stub_kernels["harl_mlp_bwd_dx_dw"]} == {want}, mode
    from harl_amd.buffers import rng_sync
    from harl_amd.nets import _bwd_fused_mode
    rng_sync()  # (the recorded updates' deferred generator advances: nothing stays pending for the tests after this one)
    monkeypatch.setenv("HARL_BWD_FUSED", "fillers")
    with pytest.raises(ValueError):
        _bwd_fused_mode(819200)
