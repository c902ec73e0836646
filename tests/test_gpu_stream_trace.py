"""-m gpu: the stream schedule of OnPolicyHARunner.train() -- which stream every launch is enqueued on, and every stream / event
operation between them, in the host's order -- against the traces recorded before that schedule was decided in one place
(tests/golden/stream_traces.json, tools/stream_trace.py).  The launch traces of tests/test_launch_trace_cpu.py are recorded on
device "cpu", where every stream branch is off; these run the real kernels of existing goldens at their own small shapes, two
``prep_training(); train()`` rounds each (the second shows that the streams are kept, not created again)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("stream_trace", os.path.join(ROOT, "tools", "stream_trace.py"))
ST = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ST)

CRITIC_LOSS = ("harl_update_fwd_critic", "harl_update_last_critic", "harl_critic_head_loss")
ACTOR_LOSS = ("harl_update_fwd_actor", "harl_update_last_actor", "harl_actor_head_loss", "harl_actor_head_loss_ls",
              "harl_md_head_loss", "harl_cat_head_loss")


@pytest.fixture(scope="module")
def traces():
    return ST.LT.normalise(ST.all_traces())


def test_stream_traces_equal_the_recorded_ones(traces):
    with open(os.path.join(ROOT, "tests", "golden", "stream_traces.json")) as f:
        want = json.load(f)
    diff = ST.compare(want, traces)
    assert not diff, "\n".join(diff)


def _rounds(trace):
    """Per train() call the launches as (position, stream, entry point)."""
    out = []
    for i, e in enumerate(trace):
        if e == ["train"]:
            out.append([])
        elif len(e) == 2 and isinstance(e[1], str):
            out[-1].append((i, e[0], e[1].split(":")[0]))
    return out


def _loss_runs(launches):
    """"A" / "C" per run of consecutive actor / critic loss launches: "CA" is critic first, "AC" critic last."""
    kinds = ["A" if n in ACTOR_LOSS else "C" for _, _, n in launches if n in ACTOR_LOSS or n in CRITIC_LOSS]
    return "".join(k for i, k in enumerate(kinds) if i == 0 or kinds[i - 1] != k)


def test_the_matrix_reaches_every_branch_of_the_schedule(traces):
    seen = set()
    for name, trace in traces.items():
        rounds = _rounds(trace)
        assert len(rounds) == 2, name
        assert {s for rnd in rounds for _, s, _ in rnd} == {s for _, s, _ in rounds[0]}, name  # no stream of the second round is new
        for rnd in rounds:
            runs = _loss_runs(rnd)
            critic_on = {s for _, s, n in rnd if n in CRITIC_LOSS}
            assert len(critic_on) == 1, name
            if runs.startswith("CA") and critic_on == {"main"}:
                seen.add("critic first, main stream")
            if runs.startswith("CA") and critic_on != {"main"}:
                seen.add("critic first, own stream")
            if "ACAC" in runs and critic_on != {"main"}:
                seen.add("critic one epoch behind each agent")
            if runs.endswith("AC") and "C" not in runs[:-1] and critic_on == {"main"}:
                seen.add("critic last")
            losses = [i for i, _, n in rnd if n in ACTOR_LOSS]
            assert losses, name  # (every configuration of the matrix updates at least one actor per round)
            logp = [(i, s) for i, s, n in rnd if n.endswith("_head_logp") and s != "main"]
            side = {s for i, s in logp if i < losses[0]}
            if side:
                seen.add("side stream")
            if any(s not in side and losses[0] < i < losses[-1] for i, s in logp):
                seen.add("post stream")
    assert seen == {"critic first, main stream", "critic first, own stream", "critic one epoch behind each agent", "critic last",
                    "side stream", "post stream"}, seen
