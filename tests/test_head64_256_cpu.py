"""HARL_HEAD64_256 on the host side (harl_amd/configs.py, the constructors): unset, every text is the one it was; set, the specs
of tests/test_gpu_head64_256.py are accepted, the new refusals answer with texts of their own and everything else keeps its own."""
import pytest
import torch

from harl_amd.configs import GAUSS_WIDE_REFUSALS, HEAD64_256_REFUSALS, MIXED_256_REFUSALS, unsupported_reason
from tests.gpu_checks import Box, Discrete, default_args
from tests.test_multidiscrete_cpu import stub_kernels  # noqa: F401  (fixture: the C-ABI dispatcher replaced by a recorder)

ALL = ("HARL_HEAD64_256", "HARL_GAUSS_WIDE", "HARL_MIXED_256", "HARL_ACT_256")
WIDER = "action heads wider than 32 (Categorical: 64) are not implemented (act_dim = 40)"
NOT_MIXED = "hidden widths [128, 256]: 256-wide layers cannot be mixed with narrower ones"
# the constructors' own wording where it always differed from unsupported_reason's
CTOR = {WIDER: "action heads wider than 32 (Categorical: 64) are not instantiated",
        NOT_MIXED: "hidden width 256: all layers must be 256 wide, feed-forward, inputs <= 512"}
# (switches set, algo, hidden_sizes, space, act_dim, activation, expected reason)
TABLE = [
    # unset: the three texts of today
    ("", "happo", [256, 256], "Discrete", 40, "relu", None),  # (accepted, and fails at its first launch: test_runtime_gate below)
    ("HARL_MIXED_256", "happo", [128, 256], "Discrete", 40, "relu", MIXED_256_REFUSALS["head"]),
    ("HARL_GAUSS_WIDE", "happo", [256, 256], "Box", 40, "relu", GAUSS_WIDE_REFUSALS["panel"]),
    # set: the accepted cases
    ("HARL_HEAD64_256", "happo", [256, 256], "Discrete", 33, "relu", None),
    ("HARL_HEAD64_256", "mappo", [256, 256, 256], "Discrete", 64, "relu", None),
    ("HARL_HEAD64_256 HARL_MIXED_256", "haa2c", [128, 256], "Discrete", 48, "relu", None),
    ("HARL_HEAD64_256 HARL_GAUSS_WIDE", "happo", [256, 256], "Box", 33, "relu", None),
    ("HARL_HEAD64_256 HARL_GAUSS_WIDE", "haa2c", [256, 256], "Box", 64, "relu", None),
    ("HARL_HEAD64_256 HARL_GAUSS_WIDE HARL_MIXED_256", "mappo", [256, 128], "Box", 40, "relu", None),
    # each new refusal
    ("HARL_HEAD64_256", "hatrpo", [256, 256], "Discrete", 40, "relu", HEAD64_256_REFUSALS["hatrpo"]),
    ("HARL_HEAD64_256 HARL_ACT_256", "happo", [256, 256], "Discrete", 40, "tanh", HEAD64_256_REFUSALS["act"]),
    # what keeps the text it has
    ("HARL_HEAD64_256", "happo", [256, 256], "Box", 40, "relu", WIDER),  # (alone the switch leaves Box refused)
    ("HARL_HEAD64_256 HARL_MIXED_256", "happo", [128, 256], "Box", 40, "relu", MIXED_256_REFUSALS["head"]),  # (constructor: WIDER's, first)
    ("HARL_HEAD64_256", "happo", [128, 256], "Discrete", 40, "relu", NOT_MIXED),
    ("HARL_HEAD64_256 HARL_GAUSS_WIDE", "hatrpo", [256, 256], "Box", 40, "relu", GAUSS_WIDE_REFUSALS["hatrpo"]),
    ("HARL_HEAD64_256 HARL_GAUSS_WIDE HARL_ACT_256", "happo", [256, 256], "Box", 40, "tanh", GAUSS_WIDE_REFUSALS["act"]),
    ("HARL_HEAD64_256 HARL_GAUSS_WIDE", "happo", [256, 256], "Box", 65, "relu", GAUSS_WIDE_REFUSALS["n"]),
]


@pytest.mark.parametrize("env,algo,hs,space,n,act,want", TABLE, ids=[f"{r[0] or 'unset'}-{r[1]}-{r[2]}-{r[3]}{r[4]}-{r[5]}" for r in TABLE])
def test_reason_and_constructor(monkeypatch, stub_kernels, env, algo, hs, space, n, act, want):  # noqa: F811
    from harl_amd.hatrpo import HATRPO
    from harl_amd.nets import StochasticPolicy
    for v in ALL:
        monkeypatch.setenv(v, "1") if v in env.split() else monkeypatch.delenv(v, raising=False)
    args = dict(model=dict(hidden_sizes=list(hs), activation_func=act), algo={})
    assert unsupported_reason(algo, args, obs_dim=19, act_space_name=space, act_dim=n) == want
    sp = Discrete(n) if space == "Discrete" else Box((n,))
    trpo = dict(kl_threshold=0.01, ls_step=10, accept_ratio=0.5, backtrack_coeff=0.8) if algo == "hatrpo" else {}
    build = lambda: (HATRPO if trpo else StochasticPolicy)(default_args(hs, activation_func=act, **trpo), Box((19,)), sp, torch.device("cpu"))  # noqa: E731
    if want is None:
        net = build()
        assert net.wide_head and net.head64_256 == ("HARL_HEAD64_256" in env and hs[-1] == 256)
    else:
        with pytest.raises(NotImplementedError) as e:
            build()
        assert str(e.value) in (want, CTOR.get(want), CTOR[WIDER] if space == "Box" and "HARL_GAUSS_WIDE" not in env else want)


def test_runtime_gate(monkeypatch, stub_kernels):  # noqa: F811
    """Unset, Discrete(40) on all-256 passes the constructor and ends at its first head launch with the library's text, as before."""
    from harl_amd.nets import StochasticPolicy
    monkeypatch.delenv("HARL_HEAD64_256", raising=False)
    net = StochasticPolicy(default_args([256, 256]), Box((19,)), Discrete(40), torch.device("cpu"))
    net._ensure_ws(64)
    with pytest.raises(RuntimeError, match=r"harl_actor_head_logp failed \(-2\): actor head: hidden width must be 64 or 128"):
        net.head_logp(64)
