"""HARL_TRPO_CAT_WIDE_256 on the host side: it lifts HATRPO's refusal only next to HARL_TRPO_CAT_WIDE=1 and HARL_CAT_WIDE_256=1, every
other refusal keeps its text, and a Fisher-vector product on such a trunk launches the grouped tangent and no harl_mlp_linear."""
import pytest

from harl_amd.configs import CAT_WIDE_REFUSALS
from tests.gpu_checks import Discrete
from tests.test_cat_wide_256_cpu import _build, _reason
from tests.test_hatrpo_cpu import TRPO, _fvp_calls
from tests.test_multidiscrete_cpu import stub_kernels  # noqa: F401  (fixture: the C-ABI dispatcher replaced by a recorder)

ALL = ("HARL_TRPO_CAT_WIDE", "HARL_CAT_WIDE_256", "HARL_TRPO_CAT_WIDE_256", "HARL_MIXED_256", "HARL_TRPO_MIXED_256")
# (switches that are on, hidden sizes, HATRPO's refusal or None).  Truly alone the new switch does nothing: HATRPO answers as with
# no switch at all, with the text that comes first in cat_wide_reason's order (the opt-in of HARL_TRPO_CAT_WIDE)
CASES = [(ALL, [256, 256], None), (ALL, [256, 128], None), (ALL[:2] + ALL[3:], [256, 256], "panel"),
         ((ALL[0], ALL[2]), [256, 256], "panel"), (ALL[2:3], [256, 256], "hatrpo"), ((), [256, 256], "hatrpo")]


def _set(monkeypatch, on):
    for v in ALL:
        monkeypatch.setenv(v, "1" if v in on else "0")


@pytest.mark.parametrize("on,hs,want", CASES, ids=[f"{'+'.join(v[5:] for v in c[0]) or 'none'}-{c[1]}" for c in CASES])
def test_refusal_follows_the_switches(monkeypatch, stub_kernels, on, hs, want):  # noqa: F811
    from harl_amd.hatrpo import HATRPO
    _set(monkeypatch, on)
    want = want and CAT_WIDE_REFUSALS[want]
    assert _reason("hatrpo", 100, hs) == want
    assert _reason("happo", 100, hs) == (None if ALL[1] in on else CAT_WIDE_REFUSALS["panel"])  # (the new switch is HATRPO's alone)
    if want is None:
        t = _build(100, hs, cls=HATRPO, **TRPO)
        assert t.actor.cat_wide and t.actor.panel
    else:
        with pytest.raises(NotImplementedError) as e:
            _build(100, hs, cls=HATRPO, **TRPO)
        assert str(e.value) == want


def test_fvp_launches_on_a_panel_trunk(monkeypatch, stub_kernels):  # noqa: F811
    _set(monkeypatch, ALL)
    t, n = _fvp_calls(stub_kernels, [256, 256], 44, Discrete(300))
    assert n["harl_mlp_rect_linear_groups"] == 1 and n["harl_mlp_rect_tangent_groups"] == 1 and n["harl_cat_head_fvp"] == 1
    assert "harl_mlp_linear" not in n and stub_kernels["harl_cat_head_fvp"][0][2] is None  # (zd_b = NULL: one image per group)
    assert len(t._tangent_ws["cat_zd"]) == 1 and len(t._tangent_ws["cat_zd"][0]) == 3
