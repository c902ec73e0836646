"""The first-layer launch route of a network (nets._FlatNet._first_launch) and what it does with the normalised-input image,
host side without a GPU (C-ABI calls recorded instead of executed): the launch traces of whole train() calls against the ones
recorded before the route was decided in one place (tests/golden/launch_traces.json, tools/launch_trace.py), and the image
contract between prepare_x0n / x0n_multi_item and the forward that follows them.  The recorded matrix also holds the routes of
the backward (nets._FlatNet._backward_route; configurations 15 and up were recorded before that one was decided in one place):
BACKWARD_REACHES names what each configuration must go on launching.  Configurations 33 and up were recorded before an action
head's launches moved into nets.StochasticPolicy -- the heads of a train() no earlier configuration has, and the second kind of
configuration (LT.ACTOR_CONFIGS: the rollout entry points, update() on a gathered sample, the pieces of HATRPO's update):
HEAD_REACHES names the head launch each of them must go on reaching.  Configurations 60 and up, and 46, were recorded before
the route of an optimiser step was decided in one place (nets._FlatNet._step_route) -- the values of HARL_FUSED_UPDATE, the
callers and the row orders nothing earlier takes: STEP_REACHES names the loss launch each must go on reaching."""
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
    steps, step_route = set(), _FlatNet._step_route

    def step_spy(self, idx_is_none, seq_is_none, train):
        r = step_route(self, idx_is_none, seq_is_none, train)
        steps.add((r.kind, r.backward, idx_is_none, seq_is_none, train, type(self).__name__))
        return r
    monkeypatch.setattr(_FlatNet, "_step_route", step_spy)
    got = LT.normalise({k: LT.run_config(k, monkeypatch) for k in (*LT.CONFIGS, *LT.ACTOR_CONFIGS)})
    diff = LT.compare(want, got)
    assert not diff, "\n".join(diff)
    # ... and the matrix still reaches every route: by the launches in the traces, and by what the route function answered
    launched = {c[0] for t in got.values() for c in t}
    assert set(FIRST_LAUNCH.values()) <= launched
    assert {a[0] for a in asked} == set(FIRST_LAUNCH)
    assert {a[2] for a in asked} == {True, False} and {a[3] for a in asked} == {True, False}
    assert {a[:2] for a in asked} == {("act", "cached"), ("panel", "cached"), ("trunk", "cached"), ("wide", "cached"),
                                      ("fused2x", "cached_identity"), ("fused2", "clobbers"), ("input", "clobbers")}
    # ... and every route of the backward (nets._backward_route) and every head launch (HEAD_REACHES): each configuration
    # recorded for one still launches it
    for name, reaches in (*BACKWARD_REACHES.items(), *HEAD_REACHES.items(), *STEP_REACHES.items()):
        for r in reaches:
            entry_tag, pred = (r, None) if isinstance(r, str) else r
            hits = _launches(got[name], entry_tag)
            assert hits and (pred is None or any(pred(a) for a in hits)), (name, entry_tag)
    # ... and every route of an optimiser step (nets._step_route): by what the route function answered -- each (kind, backward)
    # pair that exists, both values of each argument, both network classes -- and by the loss launches a configuration stays off
    assert {s[:2] for s in steps} == {("fused", "layers"), ("fused", "recompute"), ("fused", "none"), ("last", "layers"),
                                      ("layers", "layers"), ("layers", "none")}
    assert all({s[i] for s in steps} == {True, False} for i in (2, 3, 4))
    assert {s[5] for s in steps if s[0] != "layers"} == {s[5] for s in steps if s[0] == "layers"} == {"StochasticPolicy", "VNet"}
    for name, off in STEP_AVOIDS.items():
        hit = {c[0] for c in got[name] if c[0].startswith(off)}
        assert not hit, (name, hit)
    assert not _launches(got["16_h128x2_obs40_bwd_fused"], "harl_mlp_bwd_dx_dw:bwd_full")       # 64-wide image: the layer kernels
    assert not _launches(got["16_h128x2_obs40_bwd_fused"], "harl_mlp_bwd_dx_dw:bwd_full_dw1")
    assert not _launches(got["22_gru64_dw6"], "harl_mlp_dw_partials_multi:dw_gru")
    t24 = got["24_gru64_n2"]  # two GRU layers: two gate-gradient launches per backward
    assert len(_launches(t24, "harl_mlp_dw_partials_multi:dw_gru")) == 2 * len(_launches(t24, "harl_mlp_dw_partials:dw_input"))
    one_layer = {c[0] for c in got["32_h128_obs40_1layer"]}  # L = 1: no hidden layer to go back through
    assert not one_layer & {"harl_mlp_bwd_dx", "harl_mlp_bwd_dx_dw", "harl_mlp_bwd_trunk"}
    assert not _launches(got["32_h128_obs40_1layer"], "harl_mlp_dw_partials:dw_hidden")
    # the three kinds of head (plain, MultiDiscrete groups, wide Categorical) under each of log-prob, loss and Fisher-vector
    # product -- MultiDiscrete has no FVP (HATRPO asserts against it) -- and both KL sums
    heads = {n: {c[0] for c in got[n]} for n in HEAD_REACHES}
    for what in ("logp", "loss", "fvp"):
        kinds = ("actor", "cat") if what == "fvp" else ("actor", "md", "cat")
        assert all(any(f"harl_{kind}_head_{what}" in h for h in heads.values()) for kind in kinds), what
    assert not any("harl_md_head_fvp" in h for h in heads.values())
    assert all(any(kl in h for h in heads.values()) for kl in ("harl_trpo_kl_sum", "harl_cat_kl_sum"))
    # ... exactly one of them per evaluation: a head of one kind never launches a kernel of another
    for name, (_, _, (space, n), _, _) in LT.ACTOR_CONFIGS.items():
        kind = "md" if space == "MultiDiscrete" else "cat" if space == "Discrete" and n > 64 else "actor"
        other = {f"harl_{k}_head_{w}" for k in ("actor", "md", "cat") for w in ("logp", "loss", "fvp") if k != kind}
        other |= {"harl_trpo_kl_sum" if kind == "cat" else "harl_cat_kl_sum"}
        assert not heads[name] & other, (name, heads[name] & other)
        assert (kind == "actor") == ("harl_mlp_linear:md_linear" not in {f"{c[0]}:{c[1] or ''}" for c in got[name]}), name


def _launches(trace, entry_tag):
    """Argument lists of the calls ``entry:tag`` of a full trace."""
    return [c[2] for c in trace if f"{c[0]}:{c[1] or ''}" == entry_tag]


# configuration -> the launches its backward was recorded to reach: "entry:tag", or ("entry:tag", predicate on the arguments
# of one such call).  Argument positions as in include/harl_hip.h: harl_mlp_bwd_dx_dw(.., dz_prev [8], x0n [9], .., fill [14]),
# harl_gru_bwd(.., dx [19]), harl_mlp_dw_partials(A, a_rows [1], lda, HO [3], B, b_rows [5], ldb [6], ..)
BACKWARD_REACHES = {
    "15_h128x3_bwd_fused": [("harl_mlp_bwd_dx_dw:bwd_full", lambda a: a[8] is not None and a[9] is None),
                            ("harl_mlp_bwd_dx_dw:bwd_full_dw1", lambda a: a[8] is None and a[10] == 32)],
    "16_h128x2_obs40_bwd_fused": [("harl_mlp_bwd_dx:bwd_dx_dw1", lambda a: a[10] == 64), "harl_mlp_dw_partials:dw_hidden"],
    "17_h128x2_obs40_bwd_k64": [("harl_mlp_bwd_dx_dw:bwd_full", lambda a: a[8] is not None and a[6] == 128),  # writes dz_1
                                ("harl_mlp_dw_partials:dw_input", lambda a: a[10] == 64)],
    "18_h128x2_nofill": [("harl_mlp_bwd_dx_dw:bwd_full_dw1", lambda a: a[14] == 0)],
    "19_h128x2_fill": [("harl_mlp_bwd_dx_dw:bwd_full_dw1", lambda a: a[14] == 2)],
    "14b_h128x2_bwd_fused": [("harl_mlp_bwd_dx_dw:bwd_full_dw1", lambda a: a[14] == 1)],
    "20_h128x2_fused1": ["harl_update_bwd:update_bwd"],
    "21_gru64_layers": [("harl_gru_bwd:gru_bwd", lambda a: a[19] is not None and a[9] == 64), "harl_mlp_dw_partials_multi:dw_gru",
                        "harl_mlp_dw_partials:dw_input"],
    "22_gru64_dw6": ["harl_gru_dw6:dw_gru", ("harl_gru_bwd:gru_bwd", lambda a: a[19] is None),
                     ("harl_mlp_dw_partials_multi_v:dw_trunk", lambda a: a[0] == 2)],  # the MLP's problems only
    "12_h64x2_obs128_gru": [("harl_mlp_dw_partials_multi_v:dw_trunk", lambda a: a[0] == 8)],  # ... with the six gate blocks
    "23_gru128": ["harl_gru_cell_bwd:gru_cell_bwd", "harl_mlp_dw_partials_multi:dw_gru", ("harl_mlp_bwd_dx:bwd_dx_dw1", lambda a: a[5] == 128)],
    "24_gru64_n2": ["harl_mlp_linear:gru_gi_bwd", "harl_gru_cell_bwd:gru_cell_bwd", "harl_mlp_dw_partials_multi:dw_gru"],
    "25_disc50": [("harl_mlp_dw_partials:dw_head", lambda a: a[1] == 0 and a[3] == 64)],  # the ATL(64) image of dhead
    "26_obs520": [("harl_mlp_dw_partials:dw_input", lambda a: a[5] == 1 and a[6] == 520)],  # B = the gathered rows
    "27_h64x3_obs128": [("harl_mlp_bwd_trunk:bwd_trunk", lambda a: a[2] == 2 and a[12][2].endswith(".dz[2]+0"))],  # the spare dz buffer
    "31_mappo_gru": ["harl_gru_bwd:gru_bwd", "harl_mlp_bwd_trunk:bwd_trunk", "harl_mlp_dw_partials_multi_v:dw_trunk"],
    "32_h128_obs40_1layer": [("harl_mlp_dw_partials:dw_input", lambda a: a[10] == 32)],
    "10_h256x2": ["harl_mlp_panel_bwd:bwd_panel"],
    "11_h128x2_tanh": ["harl_act_bwd:act_bwd"],
}


def _padded(valid: int, pad: int):
    """Predicate: the (m_valid, m_pad) pair at argument positions ``valid`` / ``pad`` is that of a padded recurrent batch."""
    return lambda a: 0 < a[valid] < a[pad]


def _trpo(clip: int, ent: int, mode: int, valid: int):
    """Predicate: HATRPO's form of a loss launch -- mode 1, clip and entropy coefficient zero, no log-prob output (the argument
    after m_pad); ``valid``: position of m_valid."""
    return lambda a: a[mode] == 1 and a[clip] == 0.0 and a[ent] == 0.0 and a[valid + 2] is None


# configuration -> the head launches it was recorded to reach, as in BACKWARD_REACHES.  Argument positions as in
# include/harl_hip.h: harl_actor_head_logp(.., actions [10], avail, logp_out [12], old_logp, factor, agg, head_out [16], m_valid
# [17], m_pad), harl_actor_head_loss(.., clip [20], ent [21], agg, trpo [23], m_valid [24], m_pad, logp_out [26], .., dw_part
# [30], n_wg), harl_actor_head_fvp(.., avail [15], m_valid [16], m_pad), harl_md_head_logp(.., head_out [13], m_valid [14],
# m_pad), harl_md_head_loss(.., ent_scale [16], clip, ent, agg, mode [20], m_valid [21], ..), harl_cat_head_logp(.., head_out
# [12], m_valid [13], m_pad), harl_cat_head_loss(.., clip [13], ent [14], mode [15], m_valid [16], m_pad, logp_out [18], ..),
# harl_cat_head_fvp(.., avail [7], m_valid [8], m_pad), harl_update_fwd_actor(.., clip [22], ent, agg, trpo [25], ..)
_HATRPO_PLAIN = [("harl_actor_head_loss:actor_head_loss", lambda a: _trpo(20, 21, 23, 24)(a) and a[30] is None and a[31] == 0),
                 "harl_actor_head_fvp:actor_head_fvp", ("harl_actor_head_logp:actor_head_logp", lambda a: a[12] is None and a[16] is not None),
                 "harl_trpo_kl_sum:trpo_kl_sum"]
_HATRPO_CAT = [("harl_cat_head_loss:cat_head_loss", _trpo(13, 14, 15, 16)), "harl_cat_head_fvp:cat_head_fvp",
               ("harl_cat_head_logp:cat_head_logp", lambda a: a[8] is None and a[12] is not None), "harl_cat_kl_sum:cat_kl_sum"]
HEAD_REACHES = {
    "33_md_train": [("harl_md_head_loss:md_head_loss", lambda a: a[23] is not None and a[20] == 0),  # epoch 0 emits log pi_old
                    ("harl_md_head_logp:md_head_logp", lambda a: a[11] is not None)],                 # the factor pass
    "34_gru64_discrete100": [("harl_cat_head_loss:cat_head_loss", lambda a: a[16] > 0 and a[17] >= a[16]),
                             ("harl_cat_head_logp:cat_head_logp", lambda a: a[14] > 0)],
    "35_haa2c": [("harl_update_fwd_actor:update_fwd", lambda a: a[25] == 2)],
    "40_happo_md": [("harl_md_head_logp:md_head_logp", lambda a: a[13] is not None and (a[14], a[15]) == (0, 0)),
                    ("harl_dist_rows:dist_rows", lambda a: a[10] == 2 and a[9] is not None),
                    ("harl_md_head_loss:md_head_loss", lambda a: a[20] == 0 and a[16] is not None)],
    "41_happo_gru64_md": [("harl_md_head_logp:md_head_logp", _padded(14, 15)), ("harl_md_head_loss:md_head_loss", _padded(21, 22)),
                          "harl_critic_head_values:"],
    "42_happo_gru64x2_box": [("harl_actor_head_logp:actor_head_logp", _padded(17, 18)),
                             ("harl_actor_head_loss:actor_head_loss", lambda a: _padded(24, 25)(a) and a[30] is not None),
                             "harl_critic_head_values:"],
    "43_happo_gru64_discrete200": [("harl_cat_head_logp:cat_head_logp", _padded(13, 14)), ("harl_cat_head_loss:cat_head_loss", _padded(16, 17))],
    "44_happo_discrete64": [("harl_actor_head_loss:actor_head_loss", lambda a: a[30] is None and a[31] > 0 and a[23] == 0),  # wide_head:
                            ("harl_mlp_dw_partials:dw_head", lambda a: a[3] == 64),                   # ... the separate dW pass
                            ("harl_actor_head_logp:actor_head_logp", lambda a: (a[17], a[18]) == (0, 0)), "harl_update_values:update_values"],
    "45_haa2c_box": [("harl_update_fwd_actor:update_fwd", lambda a: a[25] == 2), "harl_update_logp:update_logp"],
    "46_happo_box_logp": [("harl_actor_head_loss:actor_head_loss", lambda a: a[30] is not None and a[23] == 0)],  # (its passes: STEP_REACHES)
    "50_hatrpo_box": _HATRPO_PLAIN + ["harl_update_logp:update_logp"],
    "51_hatrpo_h64_discrete5": _HATRPO_PLAIN + [("harl_actor_head_fvp:actor_head_fvp", lambda a: a[13] == 1 and a[15] is not None)],
    "52_hatrpo_gru64_box": _HATRPO_PLAIN + ["harl_gru_tangent:gru_tangent", ("harl_actor_head_fvp:actor_head_fvp", _padded(16, 17)),
                                            ("harl_actor_head_loss:actor_head_loss", _padded(24, 25))],
    "53_hatrpo_gru128_discrete5": _HATRPO_PLAIN + [("harl_actor_head_fvp:actor_head_fvp", _padded(16, 17))],
    "54_hatrpo_discrete200": _HATRPO_CAT + [("harl_cat_head_fvp:cat_head_fvp", lambda a: a[7] is not None and (a[8], a[9]) == (0, 0))],
    "55_hatrpo_gru64_discrete130": _HATRPO_CAT + ["harl_gru_tangent:gru_tangent", ("harl_cat_head_fvp:cat_head_fvp", _padded(8, 9)),
                                                  ("harl_cat_head_logp:cat_head_logp", _padded(13, 14))],
    "56_hatrpo_h256_box": _HATRPO_PLAIN + ["harl_head_dw_rows256:dw_head", "harl_mlp_panel_tangent:tangent_panel"],
    "57_hatrpo_tanh_box": _HATRPO_PLAIN + ["harl_act_ln_tangent:act_ln_tangent"],
}


# configuration -> the loss launches (and the launches that follow from the same route) its optimiser steps and forward-only
# passes were recorded to reach, as in BACKWARD_REACHES, with a predicate where an argument carries the route.  Argument
# positions as in include/harl_hip.h: harl_update_fwd_actor(x0n, M, D, H [3], .., xh1 [31], rmask1, rstd1),
# harl_update_fwd_critic(x0n, M, D, H [3], .., xh1 [21], ..), harl_update_last_actor(x, M, H [2], .., idx [12], ..),
# harl_update_last_critic(x, M, H [2], .., idx [7], ..)
_FWD_A, _FWD_C = "harl_update_fwd_actor:update_fwd", "harl_update_fwd_critic:update_fwd_critic"
_LAST_A, _LAST_C = "harl_update_last_actor:update_last", "harl_update_last_critic:update_last_critic"
_LOSS_A, _LOSS_C = "harl_actor_head_loss:actor_head_loss", "harl_critic_head_loss:critic_head_loss"
_LOGP, _HEAD_LOGP = "harl_update_logp:update_logp", "harl_actor_head_logp:actor_head_logp"
_HYBRID = [(_FWD_A, lambda a: a[31] is not None and a[32] is not None and a[33] is not None),  # layer 1's activation record
           (_FWD_C, lambda a: a[21] is not None and a[22] is not None and a[23] is not None)]
STEP_REACHES = {
    "01_h128x2": _HYBRID + [_LOGP],
    "02_h128x2_obs40": [_LOSS_A, _LOGP, (_FWD_C, lambda a: a[2] == 60 and a[21] is not None)],  # the ACTOR step does not fit the LDS
    "03_h128x3": [(_LAST_A, lambda a: a[12] is None and a[2] == 128), (_LAST_C, lambda a: a[7] is None), _HEAD_LOGP],
    "04_h128x3_mb2": [(_LAST_A, lambda a: a[12] is not None), (_LAST_C, lambda a: a[7] is not None)],
    "05_h128_64": [_LOSS_A, _LOSS_C, _HEAD_LOGP],
    "14a_h128x2_logp": [_LOSS_A, _LOSS_C, _LOGP],
    "20_h128x2_fused1": [(_FWD_A, lambda a: a[31] is None and a[32] is None and a[33] is None),  # "recompute": nothing to leave
                         (_FWD_C, lambda a: a[21] is None and a[22] is None and a[23] is None), "harl_update_bwd:update_bwd", _LOGP],
    "60_mappo_share": _HYBRID,
    "61_mappo_share_mb2": [(_LOSS_A, lambda a: a[12] is not None), _LOSS_C],  # gathered rows (idx [12]): the layer kernels
    "62_h128x2_fused_actor": [(_FWD_A, lambda a: a[31] is None), "harl_update_bwd:update_bwd", _LOSS_C, _LOGP],
    "63_h128x2_fused0": [_LOSS_A, _LOSS_C, _HEAD_LOGP],
    "64_h128x2_mb2": [_LOSS_A, _LOSS_C, _LOGP],  # two layers, both fused by the first launch: nothing left for "last"
    "65_h128x2_obs40_mb2": [(_LAST_A, lambda a: a[12] is not None and a[2] == 128), (_LAST_C, lambda a: a[7] is not None), _LOGP],
    "66_h128x3_fused1": [_LOSS_A, _LOSS_C, _HEAD_LOGP],
    "67_h64x2": [(_FWD_A, lambda a: a[3] == 64 and a[31] is not None), (_FWD_C, lambda a: a[3] == 64 and a[21] is not None), _LOGP],
    "68_h128x2_act12": [_LOSS_A, _HEAD_LOGP, (_FWD_C, lambda a: a[21] is not None)],  # a head of more than 8 outputs
    "46_happo_box_logp": [_LOSS_A, _LOGP, "harl_update_values:update_values"],
}
# ... and the entry points (by prefix) none of its launches may start with
STEP_AVOIDS = {
    "14a_h128x2_logp": ("harl_update_fwd", "harl_update_last", "harl_update_bwd"),
    "20_h128x2_fused1": ("harl_mlp_bwd_dx", "harl_update_last"),
    "61_mappo_share_mb2": ("harl_update_fwd", "harl_update_last", "harl_update_bwd"),
    "62_h128x2_fused_actor": ("harl_update_fwd_critic", "harl_update_last"),
    "63_h128x2_fused0": ("harl_update_",),
    "64_h128x2_mb2": ("harl_update_fwd", "harl_update_last", "harl_update_bwd"),
    "65_h128x2_obs40_mb2": ("harl_update_fwd", "harl_update_bwd", "harl_actor_head_loss", "harl_critic_head_loss"),
    "66_h128x3_fused1": ("harl_update_",),
    "68_h128x2_act12": ("harl_update_fwd_actor", "harl_update_last", "harl_update_logp"),
}


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
        kind = net._step_route(idx is None, seq is None, True).kind
        if kind == "last":
            seen["partial"] += 1
            forwards.append(lambda: net.forward_trunk(X, idx, M, upto=len(net.hidden_sizes) - 1))
        if kind == "fused":
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
