"""Launch traces of whole train() calls, host side without a GPU: every C-ABI call of two ``prep_training(); train()`` rounds
recorded instead of executed (the recorder of tests/test_multidiscrete_cpu.stub_kernels, a runner built like
tests/test_hybrid_cpu._runner), in launch order, as [entry point, tag, arguments].  Arguments are reduced by their ctypes type
in _lib.SIGNATURES: integers and floats literally, pointers to ``null`` or to the name of the persistent network tensor they
point into (``actor0.xh[1]+0``; anything else is ``P``), elements of ctypes arrays likewise.  The names are the point: a change
of the Python orchestration that hands another workspace to a kernel, or stops dropping the normalised-input image, changes the
trace, while addresses and the allocator's reuse of them do not.

    python tools/launch_trace.py --check tests/golden/launch_traces.json   # regenerate and compare (exit status 1: differs)
    python tools/launch_trace.py --write tests/golden/launch_traces.json   # per configuration: names + tags, SHA-256 of the rest (extends FIXTURE's name table)
    python tools/launch_trace.py --full a.json                             # the full traces (about 400 KB)
    python tools/launch_trace.py --diff a.json b.json                      # first differing call of two --full dumps

A second kind of configuration (ACTOR_CONFIGS) builds one actor directly and records the entry points that evaluate its action
head -- get_actions, evaluate_actions, update() on a gathered sample, the critic's get_values, the pieces of HATRPO's update --
which no train() of the first kind reaches.

tests/test_launch_trace_cpu.py runs the comparison of --check in the suite."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

MODS = ("nets", "buffers", "happo", "hatrpo", "mappo", "v_critic", "valuenorm", "runner", "gru_wide")
_SMAC = dict(obs=128, sobs=128)
_GRU = dict(_SMAC, use_recurrent_policy=True, data_chunk_length=4)
# name -> (hidden sizes, runner keywords, environment).  Between them: every first-layer launch of nets.forward_trunk, with
# and without a row-index tensor (one / two minibatches), whole trunks and trunks that stop in front of harl_update_last_*.
CONFIGS = {
    "01_h128x2": ([128, 128], {}, {}),
    "02_h128x2_obs40": ([128, 128], dict(obs=40, sobs=60), {}),
    "03_h128x3": ([128, 128, 128], {}, {}),
    "04_h128x3_mb2": ([128, 128, 128], dict(actor_num_mini_batch=2, critic_num_mini_batch=2), {}),
    "05_h128_64": ([128, 64], {}, {}),
    "06_h128_64_obs40": ([128, 64], dict(obs=40), {}),
    "07_h64x2_obs128": ([64, 64], dict(_SMAC), {}),
    "08_h64x2_obs128_layers": ([64, 64], dict(_SMAC), dict(HARL_TRUNK_FUSED="0")),
    "09_h64x3_obs128_mb2": ([64, 64, 64], dict(_SMAC, actor_num_mini_batch=2, critic_num_mini_batch=2), {}),
    "10_h256x2": ([256, 256], {}, {}),
    "11_h128x2_tanh": ([128, 128], dict(activation_func="tanh"), {}),
    "12_h64x2_obs128_gru": ([64, 64], dict(_SMAC, use_recurrent_policy=True, data_chunk_length=4), {}),
    "13_h128x2_discrete100": ([128, 128], dict(discrete=100), {}),
    "14a_h128x2_logp": ([128, 128], {}, dict(HARL_FUSED_UPDATE="logp")),
    "14b_h128x2_bwd_fused": ([128, 128], {}, dict(HARL_BWD_FUSED="1")),
    # ... and the routes of nets.backward_trunk the fifteen above do not reach (what each launches: tests/test_launch_trace_cpu.py)
    "15_h128x3_bwd_fused": ([128, 128, 128], {}, dict(HARL_BWD_FUSED="1")),
    "16_h128x2_obs40_bwd_fused": ([128, 128], dict(obs=40, sobs=60), dict(HARL_BWD_FUSED="1")),
    "17_h128x2_obs40_bwd_k64": ([128, 128], dict(obs=40, sobs=60), dict(HARL_BWD_FUSED="1", HARL_BWD_K64="1")),
    "18_h128x2_nofill": ([128, 128], {}, dict(HARL_BWD_FUSED="nofill")),
    "19_h128x2_fill": ([128, 128], {}, dict(HARL_BWD_FUSED="fill")),
    "20_h128x2_fused1": ([128, 128], {}, dict(HARL_FUSED_UPDATE="1")),
    "21_gru64_layers": ([64, 64], dict(_GRU), dict(HARL_TRUNK_FUSED="0")),
    "22_gru64_dw6": ([64, 64], dict(_GRU), dict(HARL_GRU_DW6="1")),
    "23_gru128": ([128, 128], dict(use_recurrent_policy=True, data_chunk_length=4), {}),
    "24_gru64_n2": ([64, 64], dict(_GRU, recurrent_n=2), {}),
    "25_disc50": ([128, 128], dict(discrete=50), {}),
    "26_obs520": ([128, 128], dict(obs=520, sobs=520), {}),
    "27_h64x3_obs128": ([64, 64, 64], dict(_SMAC), {}),
    "31_mappo_gru": ([64, 64], dict(_GRU, algo="mappo"), {}),
    "32_h128_obs40_1layer": ([128], dict(obs=40), {}),
    # ... and the action heads a train() above does not launch: MultiDiscrete groups, a wide Categorical behind a GRU, HAA2C's mode
    "33_md_train": ([128, 128], dict(nvec=(41, 41, 41, 30)), {}),
    "34_gru64_discrete100": ([64, 64], dict(_GRU, discrete=100), {}),
    "35_haa2c": ([128, 128], dict(algo="haa2c", a2c_epoch=2), {}),
    # ... and the optimiser-step routes (nets._FlatNet._step_route) nothing above takes: the shared actor of MAPPO as the caller,
    # HARL_FUSED_UPDATE=actor and =0, gathered rows on a two-layer network (19 inputs: the layer kernels; 40 / 60: the last layer
    # inside the loss launch), =1 on a network the one-launch step does not cover, that step at width 64, a head of more than 8 outputs
    "60_mappo_share": ([128, 128], dict(algo="mappo", share_param=True), {}),
    "61_mappo_share_mb2": ([128, 128], dict(algo="mappo", share_param=True, actor_num_mini_batch=2, critic_num_mini_batch=2), {}),
    "62_h128x2_fused_actor": ([128, 128], {}, dict(HARL_FUSED_UPDATE="actor")),
    "63_h128x2_fused0": ([128, 128], {}, dict(HARL_FUSED_UPDATE="0")),
    "64_h128x2_mb2": ([128, 128], dict(actor_num_mini_batch=2, critic_num_mini_batch=2), {}),
    "65_h128x2_obs40_mb2": ([128, 128], dict(obs=40, sobs=60, actor_num_mini_batch=2, critic_num_mini_batch=2), {}),
    "66_h128x3_fused1": ([128, 128, 128], {}, dict(HARL_FUSED_UPDATE="1")),
    "67_h64x2": ([64, 64], {}, {}),
    "68_h128x2_act12": ([128, 128], dict(act=12), {}),
}
_TRPO = dict(kl_threshold=0.01, ls_step=10, accept_ratio=0.5, backtrack_coeff=0.8)
_REC = dict(use_recurrent_policy=True)
_CAT = dict(HARL_TRPO_CAT_WIDE="1")
# The second kind, name -> (actor class, hidden sizes, action space (class name, argument), model keywords, environment): ONE actor
# built directly, and the entry points that evaluate its action head instead of a runner's train() (run_actor_config): what no
# train() of CONFIGS reaches -- the rollout entry points, update() on a gathered sample, every HATRPO launch.
ACTOR_CONFIGS = {
    "40_happo_md": ("HAPPO", [128, 128], ("MultiDiscrete", [3, 4]), {}, {}),
    "41_happo_gru64_md": ("HAPPO", [64], ("MultiDiscrete", [3, 4]), _REC, {}),
    "42_happo_gru64x2_box": ("HAPPO", [64, 64], ("Box", 3), _REC, {}),
    "43_happo_gru64_discrete200": ("HAPPO", [64], ("Discrete", 200), _REC, {}),
    "44_happo_discrete64": ("HAPPO", [128, 128], ("Discrete", 64), {}, {}),
    "45_haa2c_box": ("HAA2C", [128, 128], ("Box", 3), dict(a2c_epoch=2), {}),
    "46_happo_box_logp": ("HAPPO", [128, 128], ("Box", 3), {}, dict(HARL_FUSED_UPDATE="logp")),  # a layer-kernel step, fused get_values
    "50_hatrpo_box": ("HATRPO", [128, 128], ("Box", 3), {}, {}),
    "51_hatrpo_h64_discrete5": ("HATRPO", [64, 64], ("Discrete", 5), {}, {}),
    "52_hatrpo_gru64_box": ("HATRPO", [64, 64], ("Box", 3), _REC, {}),
    "53_hatrpo_gru128_discrete5": ("HATRPO", [128, 128], ("Discrete", 5), _REC, {}),
    "54_hatrpo_discrete200": ("HATRPO", [128, 128], ("Discrete", 200), {}, _CAT),
    "55_hatrpo_gru64_discrete130": ("HATRPO", [64], ("Discrete", 130), _REC, _CAT),
    "56_hatrpo_h256_box": ("HATRPO", [256, 256], ("Box", 3), {}, {}),
    "57_hatrpo_tanh_box": ("HATRPO", [128, 128], ("Box", 3), dict(activation_func="tanh"), {}),
}
# the switches a configuration may set: cleared around every run, so that the caller's environment does not leak into a trace
SWITCHES = ("HARL_FUSED_UPDATE", "HARL_BWD_FUSED", "HARL_BWD_K64", "HARL_TRUNK_FUSED", "HARL_GRAPH", "HARL_BWD_STREAMS",
            "HARL_GRU128", "HARL_GRU_COMPOSED", "HARL_NWG", "HARL_X0N_MULTI", "HARL_FOLD_TABLE", "HARL_ALWAYS_FOLD",
            "HARL_GRU_DW6", "HARL_TRUNK_DW_STREAM", "HARL_LIB", "HARL_TRPO_CAT_WIDE", "HARL_UNFOLD_TABLE",
            "HARL_TANGENT_ONE_LAUNCH")


def make_runner(hidden, obs=19, sobs=11, act=3, discrete=0, nvec=None, T=8, N=8, A=2, algo="happo", **over):
    """tests/test_hybrid_cpu._runner, plus a Discrete(``discrete``) or MultiDiscrete(``nvec``) action space and the runner of
    ``algo`` (``over``: a2c_epoch for "haa2c")."""
    from harl_amd.runner import RUNNER_REGISTRY
    from harl_amd.synthetic import Shapes, make_buffers
    from tests.gpu_checks import Box, Discrete, MultiDiscrete, default_args
    a = default_args(hidden, ppo_epoch=2, critic_epoch=2, **over)
    train = dict(n_rollout_threads=N, episode_length=T, use_valuenorm=True, use_linear_lr_decay=False,
                 use_proper_time_limits=True, model_dir=None, eval_interval=25, use_eval=False, log_interval=1,
                 num_env_steps=T * N * 2)
    space = MultiDiscrete(nvec) if nvec else Discrete(discrete) if discrete else Box((act,))
    r = RUNNER_REGISTRY[algo](dict(algo=algo), dict(train=train, model=dict(a), algo=dict(a)), dict(state_type="EP"),
                                 obs_spaces=[Box((obs,))] * A, share_obs_space=Box((sobs,)), act_spaces=[space] * A,
                                 device=torch.device("cpu"))
    sh = Shapes(T=T, N=N, A=A, obs_dim=obs, share_obs_dim=sobs, act_dim=sum(nvec or ()) or discrete or act,
                discrete=bool(discrete), hidden_sizes=list(hidden), nvec=list(nvec) if nvec else None)
    d = make_buffers(sh, 4)
    for ag in range(A):
        b = r.actor_buffer[ag]
        b.obs.copy_(torch.from_numpy(d.obs[ag]))
        b.actions.copy_(torch.from_numpy(d.actions[ag]))
        b.action_log_probs.copy_(torch.from_numpy(d.action_log_probs[ag]))
    return r


def networks(r):
    """{owner name: network} of a runner: every actor's and the critic's."""
    nets = {f"actor{i}": a.actor for i, a in enumerate(r.actor)}
    nets["critic"] = r.critic.critic
    return nets


def _tensors(name, v, out):
    if isinstance(v, torch.Tensor):
        if v.numel():
            out.append((v.data_ptr(), v.numel() * v.element_size(), name))
    elif isinstance(v, list):
        for i, x in enumerate(v):
            _tensors(f"{name}[{i}]", x, out)
    elif isinstance(v, dict):
        for k, x in v.items():
            _tensors(f"{name}[{k}]", x, out)


class Recorder:
    """Wraps the recorder ``stub_kernels`` installed: keeps the calls in launch order, reduced to what does not depend on
    addresses."""

    def __init__(self, monkeypatch):
        from harl_amd import _lib
        self.trace, self.nets = [], {}
        self._inner, self._sig = _lib.call, _lib.SIGNATURES
        monkeypatch.setattr(_lib, "call", self)
        for mod in MODS:
            m = __import__(f"harl_amd.{mod}", fromlist=["x"])
            if hasattr(m, "call"):
                monkeypatch.setattr(m, "call", self)

    def __call__(self, name, *args, tag=None):
        types = self._sig[name]
        assert len(types) == len(args), (name, len(types), len(args))
        names = self._names()
        self.trace.append([name, tag, [self._arg(t, a, names) for t, a in zip(types, args)]])
        return self._inner(name, *args, tag=tag)

    def _names(self):
        """(start, end, name) of every persistent tensor of the networks AS THEY ARE NOW (workspaces are reallocated when
        a larger minibatch arrives), largest first: a view resolves to the arena it lives in."""
        spans = []
        for owner, net in self.nets.items():
            for attr, v in vars(net).items():
                if not attr.startswith("_parameters") and attr != "_modules":
                    _tensors(f"{owner}.{attr}", v, spans)
        return sorted(((p, p + n, nm) for p, n, nm in spans), key=lambda s: (s[0] - s[1], s[2]))

    @staticmethod
    def _resolve(p, names):
        if not p:
            return None
        for lo, hi, nm in names:
            if lo <= p < hi:
                return f"{nm}+{p - lo}"
        return "P"

    def _arg(self, ctype, a, names):
        if isinstance(a, ctypes.Array):
            if a._type_ is ctypes.c_void_p:
                return [self._resolve(x, names) for x in a]
            return [x for x in a]
        if ctype is ctypes.c_void_p:
            return self._resolve(a, names)
        return a if isinstance(a, (int, float)) else float(a)


def run_actor_config(name, rec):
    """The head-bearing entry points of ONE actor (ACTOR_CONFIGS[name]) into ``rec.trace``: get_actions on one step's rows
    (deterministic: the stub leaves ``probs`` unwritten), evaluate_actions on all rows, then update() on the gathered sample
    (HAPPO, HAA2C) next to the critic's get_values -- or, for HATRPO, the pieces of its update that launch (_update_core itself
    pins host memory and synchronises a stream).  Recurrent: L = 3 steps of m = 8 sequences, padded to the kernels' layout."""
    import numpy as np

    import harl_amd.happo
    import harl_amd.hatrpo
    from harl_amd.nets import build_seq
    from harl_amd.v_critic import VCritic
    from tests import gpu_checks as gc
    cls, hidden, (kind, n), kw, _ = ACTOR_CONFIGS[name]
    obs_dim, sobs, cpu = 19, 11, torch.device("cpu")
    space = gc.Box((n,)) if kind == "Box" else getattr(gc, kind)(n)
    args = gc.default_args(hidden, **_TRPO, **kw)
    actor = getattr(harl_amd.hatrpo if cls == "HATRPO" else harl_amd.happo, cls)(args, gc.Box((obs_dim,)), space, device=cpu)
    net = actor.actor
    rec.nets = {"actor0": net}
    L, m = (3, 8) if net.recurrent else (1, 24)
    M, rng = L * m, np.random.default_rng(0)
    f = lambda *shape: np.ones(shape, np.float32)  # noqa: E731
    obs = rng.standard_normal((M, obs_dim)).astype(np.float32)
    act = f(M, net.act_dim) if kind == "Box" else np.zeros((M, len(n) if kind == "MultiDiscrete" else 1), np.float32)
    avail = f(M, n) if kind == "Discrete" else None
    rnn, masks = np.zeros((m, net.recurrent_n, hidden[-1]), np.float32), f(M, 1)
    old_logp = np.full((M, act.shape[1]), -2.0, np.float32)
    del rec.trace[:]
    actor.get_actions(obs[:m], rnn, masks[:m], None if avail is None else avail[:m], deterministic=True)
    # (the distribution object it returns is built from head outputs that no kernel wrote here: padded rows are compacted out
    # of an uninitialised scratch tensor, so its parameters are not validated)
    validate = torch.distributions.Distribution._validate_args
    torch.distributions.Distribution.set_default_validate_args(False)
    try:
        actor.evaluate_actions(obs, rnn, act, masks, avail, f(M, 1))
    finally:
        torch.distributions.Distribution.set_default_validate_args(validate)
    if cls != "HATRPO":
        actor.update((obs, rnn, act, masks, f(M, 1), old_logp, f(M, 1), avail, f(M, 1)))
        critic = VCritic(args, gc.Box((sobs,)), device=cpu)
        rec.nets["critic"] = critic.critic
        critic.get_values(f(M, sobs), rnn, masks)
        return
    t = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
    seq, rows, avail_rows = None, M, t(avail)
    if net.recurrent:
        HS = hidden[-1] * net.recurrent_n
        seq = build_seq(cpu, L, m, HS, h0=torch.zeros(m, HS), masks_src=t(masks))
        rows = L * seq["m_pad"]
        avail_rows = None if avail is None else torch.ones(rows, n)
    net.fold()
    actor._surrogate(t(obs), rows, t(act), t(avail), t(old_logp), torch.ones(M), None, torch.ones(M), torch.ones(M),
                     want_grad=True, seq=seq)
    actor._fvp(t(obs), rows, M, avail_rows, torch.zeros(net.n_params), seq=seq)
    head = actor._head_outputs(t(obs), rows, t(act), t(avail), reuse_trunk=True, seq=seq, avail_rows=avail_rows)
    actor._kl_sum(head, None if net.discrete else net.log_std().clone(), head, M)


def run_config(name, monkeypatch, rounds=2):
    """The trace of ``rounds`` x (prep_training(); train()) of configuration ``name`` of CONFIGS, or of the entry points of
    the one actor ``name`` of ACTOR_CONFIGS (run_actor_config).  The caller has installed the stub (the ``stub_kernels``
    fixture) on the same ``monkeypatch``."""
    hidden, kw, env = CONFIGS[name] if name in CONFIGS else (None, None, ACTOR_CONFIGS[name][4])
    with monkeypatch.context() as mp:
        for k in SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        rec = Recorder(mp)
        torch.manual_seed(3)
        if hidden is None:
            run_actor_config(name, rec)
            return rec.trace
        r = make_runner(hidden, **kw)
        rec.nets = networks(r)
        del rec.trace[:]
        for _ in range(rounds):
            r.prep_training()
            r.train()
        return rec.trace


def digest(trace):
    return hashlib.sha256(json.dumps(trace, separators=(",", ":")).encode()).hexdigest()


def call_name(c):
    """The name a recorded call goes by in the fixture's table: "entry:tag"."""
    return f"{c[0]}:{c[1] or ''}"


def summarise(traces, keep=(), name=call_name):
    """What the committed fixture keeps of the full traces (they are several hundred KB): per configuration every call's entry
    point and tag in order -- as indices into ONE table of "entry:tag" names -- and a SHA-256 of the full trace.  ``keep``: the
    name table of the fixture that is being extended; its names keep their indices (and the recorded lines their bytes), new
    names follow.  ``name``: what one entry of a trace is called in that table (tools/stream_trace.py has entries of its own)."""
    names = list(keep) + sorted({name(c) for t in traces.values() for c in t} - set(keep))
    at = {n: i for i, n in enumerate(names)}
    return dict(names=names, traces={k: dict(calls=[at[name(c)] for c in t], sha256=digest(t)) for k, t in traces.items()})


def compare(want, got, name=call_name):
    """Full traces ``got`` against the fixture ``want`` (summarise), as lines of text (empty: equal): per configuration the
    first call whose entry point or tag differs, or that only the arguments do (then: first_difference of two --full dumps)."""
    out, have = [], summarise(got, name=name)
    for k in sorted(set(want["traces"]) | set(have["traces"])):
        a, b = want["traces"].get(k), have["traces"].get(k)
        if a is None or b is None:
            out.append(f"{k}: only in the {'fixture' if b is None else 'tree'}")
            continue
        ca, cb = [want["names"][i] for i in a["calls"]], [have["names"][i] for i in b["calls"]]
        if ca != cb:
            i = next((i for i, (x, y) in enumerate(zip(ca, cb)) if x != y), min(len(ca), len(cb)))
            out.append(f"{k}: call {i} of {len(ca)} / {len(cb)}: fixture {ca[i] if i < len(ca) else '(end)'}, "
                       f"tree {cb[i] if i < len(cb) else '(end)'}")
        elif a["sha256"] != b["sha256"]:
            out.append(f"{k}: the same {len(ca)} calls with other arguments (sha256 {b['sha256'][:16]}, fixture {a['sha256'][:16]}): "
                       "write --full dumps of both trees and compare them with --diff")
    return out


def first_difference(ta, tb):
    """The first differing call of every configuration of two sets of full traces, as lines of text."""
    out = []
    for k in sorted(set(ta) | set(tb)):
        a, b = ta.get(k, []), tb.get(k, [])
        i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)
        if i is None and len(a) != len(b):
            i = min(len(a), len(b))
        if i is not None:
            out.append(f"{k}: call {i} of {len(a)} / {len(b)}\n  a: {a[i] if i < len(a) else '(end)'}\n"
                       f"  b: {b[i] if i < len(b) else '(end)'}")
    return out


def normalise(traces):
    """Through JSON and back, as the fixture went: tags and NULLs as None, every sequence a list."""
    return json.loads(json.dumps(traces))


def write_fixture(path, fx):
    """A summarise() result as the committed file: the name table, then one configuration per line."""
    with open(path, "w") as f:
        f.write('{"names": ' + json.dumps(fx["names"]) + ',\n "traces": {\n' + ",\n".join(
            f'  {json.dumps(k)}: {json.dumps(t, separators=(",", ":"))}' for k, t in fx["traces"].items()) + "\n}}\n")


def all_traces():
    import pytest
    from tests.test_multidiscrete_cpu import stub_kernels
    fixture = getattr(stub_kernels, "__wrapped__", None) or stub_kernels.__pytest_wrapped__.obj
    with pytest.MonkeyPatch.context() as mp:
        fixture(mp)
        return {k: run_config(k, mp) for k in (*CONFIGS, *ACTOR_CONFIGS)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--check", metavar="FIXTURE", help="regenerate the traces and compare them with FIXTURE")
    g.add_argument("--write", metavar="FIXTURE", help="write the fixture of this tree: names, tags and a SHA-256 per configuration")
    g.add_argument("--full", metavar="OUT", help="write the full traces of this tree")
    g.add_argument("--diff", nargs=2, metavar=("A", "B"), help="the first differing call of two --full dumps")
    a = ap.parse_args()
    lines = []
    if a.diff:
        with open(a.diff[0]) as fa, open(a.diff[1]) as fb:
            lines = first_difference(json.load(fa), json.load(fb))
    else:
        traces = normalise(all_traces())
        if a.full:
            with open(a.full, "w") as f:
                json.dump(traces, f, separators=(",", ":"))
        elif a.write:
            keep = ()
            if os.path.exists(a.write):
                with open(a.write) as f:
                    keep = json.load(f)["names"]
            fx = summarise(traces, keep)
            write_fixture(a.write, fx)
        else:
            with open(a.check) as f:
                lines = compare(json.load(f), traces)
    print("\n".join(lines) if lines else "no difference")
    return 1 if lines else 0


if __name__ == "__main__":
    sys.exit(main())
