"""The launch route of an optimiser step (nets._FlatNet._step_route), host side without a GPU: its answers against the three
predicates that used to decide it between them -- fused_update_ok, fused_last_ok and fused_hybrid, quoted below as they stood
before the route was decided in one place, combined in the order of the ladder HAPPO._forward_backward and
VCritic._forward_backward both carried -- over a sweep of networks, values of HARL_FUSED_UPDATE and kinds of pass."""
import itertools

import pytest
import torch

from tests.gpu_checks import Box, MultiDiscrete, default_args
from tests.test_backward_route_cpu import SWITCHES, _networks
from tests.test_multidiscrete_cpu import stub_kernels  # noqa: F401  (fixture)

MODES = (None, "hybrid", "logp", "1", "actor", "0")
PAIRS = {("fused", "layers"), ("fused", "recompute"), ("fused", "none"), ("last", "layers"), ("layers", "layers"), ("layers", "none")}


@pytest.fixture
def nets_(stub_kernels, monkeypatch):  # noqa: F811
    from harl_amd.nets import StochasticPolicy
    for k in SWITCHES + ("HARL_FUSED_UPDATE",):
        monkeypatch.delenv(k, raising=False)
    torch.manual_seed(7)
    out, dev = list(_networks()), torch.device("cpu")
    for hidden, in_dim in itertools.product(([128, 128], [128, 128, 128], [64, 64]), (8, 40)):  # heads the fused launches do not take
        args = default_args(hidden)
        out.append((f"{hidden}/{in_dim}/box12", StochasticPolicy(args, Box((in_dim,)), Box((12,)), dev)))
        out.append((f"{hidden}/{in_dim}/md", StochasticPolicy(args, Box((in_dim,)), MultiDiscrete([3, 4]), dev)))
    assert len(out) > 150
    return out


# ---- the conditions as the parent of this route stated them, literally (``self`` -> ``net``)
def _parent_fused_update_ok(net, idx, seq=None, train=True):
    from harl_amd import _lib
    from harl_amd.nets import VNet, _fused_update_mode
    self = net
    hs = self.hidden_sizes
    mode = _fused_update_mode()
    if self.act_id:
        return False
    if mode == "0" or (train and mode == "logp") or (train and mode == "actor" and isinstance(self, VNet)):
        return False
    if not (not self.recurrent and not self.grouped and idx is None and seq is None
            and len(hs) == 2 and hs[0] == hs[1] and hs[0] in (64, 128) and self.in_dim <= 64 and self._layers()[-1][4] <= 8):
        return False
    kind = 0 if not train else (2 if isinstance(self, VNet) else 1)
    return bool(_lib.load().harl_update_supported(self.in_dim, hs[0], self._layers()[-1][4], kind))


def _parent_fused_last_ok(net, idx, seq=None):
    from harl_amd import _lib
    from harl_amd.nets import VNet, _fused_update_mode
    self = net
    hs = self.hidden_sizes
    if _fused_update_mode() != "hybrid" or self.act_id or self.recurrent or self.grouped or self.panel:
        return False
    if seq is not None or len(hs) < 2 or hs[-1] != hs[-2] or hs[-1] not in (64, 128) or self._layers()[-1][4] > 8:
        return False
    two_fused = self._first_launch(idx is None, True).kind in ("fused2x", "fused2")
    return len(hs) >= (3 if two_fused else 2) and bool(_lib.load().harl_update_supported(0, hs[-1], self._layers()[-1][4], 2 if isinstance(self, VNet) else 1))


def _parent_fused_hybrid(net):
    from harl_amd.nets import _fused_update_mode
    return _fused_update_mode() == "hybrid"


def _parent_route(net, idx, seq, train):
    """The ladder of the two _forward_backward (fused_update_ok first, then fused_last_ok, else the layer kernels; after the
    one-launch step backward_after_fused: the layer kernels under hybrid, harl_update_bwd otherwise), and the forward-only
    passes' one question."""
    if not train:
        return ("fused" if _parent_fused_update_ok(net, idx, seq, train=False) else "layers"), "none"
    if _parent_fused_update_ok(net, idx, seq):
        return "fused", ("layers" if _parent_fused_hybrid(net) else "recompute")
    if _parent_fused_last_ok(net, idx, seq):
        return "last", "layers"
    return "layers", "layers"


def _passes(net):
    """(idx, seq, train) of the sweep: recurrent networks only with a sequence layout."""
    rows, seq = torch.arange(4), dict(L=1, m_pad=4)
    for idx, s, train in itertools.product((None, rows), (None, seq), (True, False)):
        if s is not None or not net.recurrent:
            yield idx, s, train


def test_route_is_what_the_two_predicates_and_the_ladder_decided(nets_, monkeypatch):
    from harl_amd.nets import StochasticPolicy, VNet, _StepRoute
    seen = set()
    for mode in MODES:
        if mode is None:
            monkeypatch.delenv("HARL_FUSED_UPDATE", raising=False)
        else:
            monkeypatch.setenv("HARL_FUSED_UPDATE", mode)
        for label, net in nets_:
            for idx, seq, train in _passes(net):
                got = net._step_route(idx is None, seq is None, train)
                assert isinstance(got, _StepRoute), label
                assert tuple(got) == _parent_route(net, idx, seq, train), (label, mode, idx is None, seq is None, train)
                seen.add((tuple(got), type(net)))
    assert {p for p, _ in seen} == PAIRS
    assert {c for p, c in seen if p[0] != "layers"} == {StochasticPolicy, VNet}
    # "actor": the one-launch step with the recomputing backward for actors, the layer kernels for the critic
    assert (("fused", "recompute"), VNet) in seen and StochasticPolicy._update_kind == 1 and VNet._update_kind == 2


def test_an_unknown_value_of_the_variable_is_still_refused(nets_, monkeypatch):
    monkeypatch.setenv("HARL_FUSED_UPDATE", "hybird")
    for label, net in nets_[:12]:
        for train in (True, False):
            with pytest.raises(ValueError, match="HARL_FUSED_UPDATE"):
                net._step_route(True, not net.recurrent, train)
