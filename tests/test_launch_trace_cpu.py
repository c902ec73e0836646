"""The first-layer launch route of a network (nets._FlatNet._first_launch) and what it does with the normalised-input image,
host side without a GPU (C-ABI calls recorded instead of executed): the launch traces of whole train() calls against the ones
recorded before the route was decided in one place (tests/golden/launch_traces.json, tools/launch_trace.py), and the image
contract between prepare_x0n / x0n_multi_item and the forward that follows them."""
import importlib.util
import json
import os

import pytest
import torch

from tests.gpu_checks import Box, default_args
from tests.test_multidiscrete_cpu import stub_kernels  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("launch_trace", os.path.join(ROOT, "tools", "launch_trace.py"))
LT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(LT)

# entry point of the first launch of every kind of route, in forward_trunk's order of precedence
FIRST_LAUNCH = {"act": "harl_mlp_linear_wide", "panel": "harl_mlp_panel_fwd", "trunk": "harl_mlp_fwd_trunk",
                "fused2x": "harl_mlp_fwd_fused2x", "fused2": "harl_mlp_fwd_fused2", "wide": "harl_mlp_fwd_wide",
                "input": "harl_mlp_fwd_input"}
M = 64


def test_launch_traces_equal_the_recorded_ones(stub_kernels, monkeypatch):  # noqa: F811
    from harl_amd.nets import _FlatNet
    with open(os.path.join(ROOT, "tests", "golden", "launch_traces.json")) as f:
        want = json.load(f)
    asked, route = set(), _FlatNet._first_launch

    def spy(self, idx_is_none, partial):
        r = route(self, idx_is_none, partial)
        asked.add((r.kind, r.image, idx_is_none, partial))
        return r
    monkeypatch.setattr(_FlatNet, "_first_launch", spy)
    got = LT.normalise({k: LT.run_config(k, monkeypatch) for k in LT.CONFIGS})
    diff = LT.compare(want, got)
    assert not diff, "\n".join(diff)
    # ... and the matrix still reaches every route: by the launches in the traces, and by what the route function answered
    launched = {c[0] for t in got.values() for c in t}
    assert set(FIRST_LAUNCH.values()) <= launched
    assert {a[0] for a in asked} == set(FIRST_LAUNCH)
    assert {a[2] for a in asked} == {True, False} and {a[3] for a in asked} == {True, False}
    assert {a[:2] for a in asked} == {("act", "cached"), ("panel", "cached"), ("trunk", "cached"), ("wide", "cached"),
                                      ("fused2x", "cached_identity"), ("fused2", "clobbers"), ("input", "clobbers")}


def _cases(monkeypatch):
    """(label, network, X, idx, seq) for actor 0 and the critic of configurations 1 .. 12, full-buffer rows and gathered ones."""
    torch.manual_seed(5)
    rows = torch.randperm(96)[:M].contiguous()
    for name, (hidden, kw, env) in LT.CONFIGS.items():
        if name[:2] > "12":
            continue
        with monkeypatch.context() as mp:
            for k in LT.SWITCHES:
                mp.delenv(k, raising=False)
            for k, v in env.items():
                mp.setenv(k, v)
            r = LT.make_runner(hidden, **kw)
            for who, net in (("actor", r.actor[0].actor), ("critic", r.critic.critic)):
                net.fold()
                seq = None
                if net.recurrent:
                    seq = dict(L=4, m_pad=M // 4, h0=torch.zeros(M // 4, hidden[-1]), mask_rows=torch.ones(M))
                for idx in (None, rows):
                    X = torch.randn(M if idx is None else 96, net.in_dim)
                    yield f"{name}/{who}/{'identity' if idx is None else 'gathered'}", net, X, idx, seq


def _x0n(calls) -> int:
    return len(calls.get("harl_mlp_x0n_wide", ()))


def test_prepare_x0n_leaves_nothing_to_build(stub_kernels, monkeypatch):  # noqa: F811
    """What a captured optimiser step relies on (graphs.py): after prepare_x0n the step's forward launches no image kernel --
    whole trunks, trunks that stop in front of harl_update_last_* and the one-launch step's fused_args alike -- and a route
    without an image has its cache key dropped."""
    calls, seen = stub_kernels, dict(built=0, dropped=0, partial=0, fused_args=0)
    for label, net, X, idx, seq in _cases(monkeypatch):
        forwards = [lambda: net.forward_trunk(X, idx, M, seq=seq)]
        if net.fused_last_ok(idx, seq):
            seen["partial"] += 1
            forwards.append(lambda: net.forward_trunk(X, idx, M, upto=len(net.hidden_sizes) - 1))
        if net.fused_update_ok(idx, seq):
            seen["fused_args"] += 1
            forwards.append(lambda: net.fused_args(X, M))
        for fwd in forwards:
            net.invalidate_caches()
            calls.clear()
            net.prepare_x0n(X, idx, M)
            built = _x0n(calls)
            assert built <= 1, label
            calls.clear()
            fwd()
            assert _x0n(calls) == 0, label
            if built:
                seen["built"] += 1
            else:
                seen["dropped"] += 1
                assert net._x0n_key is None, label
    assert all(seen.values()), seen


def test_x0n_multi_item_is_the_image_the_forward_reads(stub_kernels, monkeypatch):  # noqa: F811
    calls, items = stub_kernels, 0
    for label, net, X, idx, seq in _cases(monkeypatch):
        if idx is not None:
            continue
        net.invalidate_caches()
        it = net.x0n_multi_item(X, M)
        if it is None:
            continue
        items += 1
        net._x0n_key, net._x0n_src = it[0], (X, None)  # as prepare_x0n_multi installs it
        calls.clear()
        net.forward_trunk(X, None, M, for_backward=False)
        assert _x0n(calls) == 0, label
    assert items >= 8


def test_image_does_not_depend_on_a_partial_trunk(stub_kernels, monkeypatch):  # noqa: F811
    """prepare_x0n does not know whether the step behind it stops the trunk in front of the last layer (``partial``): what the
    route does with the image must not depend on it."""
    for label, net, X, idx, seq in _cases(monkeypatch):
        assert net._first_launch(idx is None, True).image == net._first_launch(idx is None, False).image, label
    # ... and beyond these networks (33 .. 64 inputs in front of an all-64 trunk: "trunk" or "fused2x" over identity rows --
    # the same image): a route either reads the image of X[idx] or drops it, whatever ``partial``
    from harl_amd.nets import VNet
    kinds = set()
    for hidden in ([64, 64], [64, 64, 64], [128, 128], [128, 64], [64, 128, 128], [256, 256]):
        for act in ("relu", "tanh"):
            for in_dim in (8, 32, 33, 40, 64, 65, 128, 512):
                if act != "relu" and 256 in hidden:
                    continue
                net = VNet(default_args(hidden, activation_func=act), Box((in_dim,)), torch.device("cpu"))
                for idx_is_none in (True, False):
                    whole, part = net._first_launch(idx_is_none, False), net._first_launch(idx_is_none, True)
                    kinds |= {whole.kind, part.kind}
                    assert (whole.image == "clobbers") == (part.image == "clobbers"), (hidden, act, in_dim, idx_is_none)
                    assert idx_is_none or "cached_identity" not in (whole.image, part.image)
    assert kinds == set(FIRST_LAUNCH)
