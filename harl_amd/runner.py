"""OnPolicyHARunner: the sequential-update training step on MI355X.

Reference: harl/runners/on_policy_ha_runner.py:11-130 (train), harl/runners/on_policy_base_runner.py:462-497
(compute / after_update), :712-763 (prep_*, save / restore).  Environment stepping (collect/insert/eval/render) is
the reference's host-side rollout loop and stays there; ``from_spaces`` builds the update-side
objects directly from the spaces, which is also what ``bench.py`` and the tests use.
"""
from __future__ import annotations

import contextlib
import os
from typing import List, NamedTuple, Optional

import torch

from . import _lib
from .buffers import OnPolicyActorBuffer, OnPolicyCriticBufferEP, OnPolicyCriticBufferFP, consume_randperm, rng_sync
from ._lib import call, ptr, stream
from .dist import Comm, shard_columns
from .happo import HAA2C, HAPPO
from .hatrpo import HATRPO
from .mappo import MAPPO
from .v_critic import VCritic
from .valuenorm import ValueNorm

ALGO_REGISTRY = {"happo": HAPPO, "hatrpo": HATRPO, "haa2c": HAA2C, "mappo": MAPPO}


class _TrainSchedule(NamedTuple):
    """The stream schedule of one OnPolicyHARunner.train() call (decided by _train_schedule, where the reasons are)."""
    critic: str          # "first" | "staggered" | "last"
    critic_stream: bool  # the critic's launches go to a stream of their own ("staggered": always; "last": never)
    side: bool           # pre-update log-prob passes that the first forward cannot supply go to the side stream
    side_ahead: bool     # ... one agent ahead of the main stream instead of all up front
    post_stream: bool    # a recurrent agent's post-update pass goes to its own stream when the next agent can await it
    last_post: bool      # the pass behind the last agent of the order runs too


def _stream(runner, name: str):
    """The runner's stream ``name`` (``_critic_stream``, ``_side_stream``, ``_post_stream``): created at first use, then kept."""
    if getattr(runner, name, None) is None:
        setattr(runner, name, torch.cuda.Stream(device=runner.device))
    return getattr(runner, name)


def _on(s):
    """Context in which launches go to stream ``s``; None: they stay on the current one (and nothing of torch.cuda is touched)."""
    return contextlib.nullcontext() if s is None else torch.cuda.stream(s)


class _StaggeredCritic:
    """The critic's update handed out one epoch at a time next to the actors' (_train_schedule, "staggered").  The global CPU
    generator keeps TWO positions: the actors', which is the generator's own between two epochs, and the critic's, kept here.
    Built at the actors' position: the critic's starts behind ``footprint``, the sizes of every draw the actors will take
    (the generator advance of torch.randperm(n) each, no permutation materialised), and the generator is left where it was.
    ``epochs``: VCritic._train_epochs, ``n_epochs`` of them; ``stream``: where they are enqueued (None: where the caller is)."""

    def __init__(self, epochs, n_epochs: int, footprint, stream):
        self.gen, self.left, self.stream = epochs, n_epochs, stream
        rng_sync()
        actor_state = torch.get_rng_state()
        for n in footprint:
            consume_randperm(n)
        rng_sync()
        self.start = self.state = torch.get_rng_state()
        torch.set_rng_state(actor_state)

    def epoch(self, after_event=None) -> None:
        """The next epoch (if one is left), ordered behind ``after_event``, drawn from the critic's position; the generator is
        back at the actors' position afterwards, also when the epoch raises."""
        if self.left <= 0:
            return
        rng_sync()
        actor_state = torch.get_rng_state()
        torch.set_rng_state(self.state)
        try:
            if after_event is not None:
                self.stream.wait_event(after_event)
            with _on(self.stream):
                next(self.gen)
            self.left -= 1
            rng_sync()
            self.state = torch.get_rng_state()
        finally:
            rng_sync()  # (the deferred advances of an epoch that raised are the critic's too)
            torch.set_rng_state(actor_state)

    def finish(self) -> None:
        """Behind the last actor: the actors must have drawn exactly the footprint; then the epochs not handed out yet.
        ``state`` is then what the in-order run leaves the generator in."""
        rng_sync()
        if not torch.equal(torch.get_rng_state(), self.start):
            raise RuntimeError("the actors' draws from the CPU generator are not what rng_footprint() announced: the staggered "
                               "critic's permutations were not drawn from the state the in-order update's critic finds")
        while self.left > 0:
            self.epoch()
        for _ in self.gen:  # (run the generator to its end)
            pass


class OnPolicyHARunner:
    # feed-forward, one-minibatch updates: the critic's chain gets a stream of its own up to this many rows per minibatch (train())
    CRITIC_STREAM_MAX_ROWS = 150_000

    def __init__(self, args: dict, algo_args: dict, env_args: Optional[dict] = None, *, obs_spaces=None,
                 share_obs_space=None, act_spaces=None, device: Optional[torch.device] = None,
                 comm: Optional[Comm] = None, envs=None, logger=None, eval_envs=None, save_dir: Optional[str] = None):
        """``args``/``algo_args`` as in examples/train.py:87-91.  Spaces must be given explicitly or through ``envs``
        (a vectorised environment with the reference's ``ShareVecEnv`` surface: ``observation_space``,
        ``share_observation_space``, ``action_space`` lists and ``reset()/step()``, envs/env_wrappers.py); this class
        does not create environments.  With an initialised process group, ``algo_args['train']['n_rollout_threads']`` is
        the GLOBAL thread count and this rank keeps its contiguous column shard."""
        self.envs, self.logger, self.eval_envs, self.save_dir = envs, logger, eval_envs, save_dir
        if envs is not None and obs_spaces is None:
            obs_spaces, act_spaces = list(envs.observation_space), list(envs.action_space)
            share_obs_space = envs.share_observation_space[0]
        if obs_spaces is None or share_obs_space is None or act_spaces is None:
            raise ValueError("OnPolicyHARunner needs obs_spaces / share_obs_space / act_spaces (no env creation here)")
        self.args = args
        self.algo_args = algo_args
        self.env_args = env_args
        self.device = torch.device(device if device is not None else "cuda:0")
        _lib.require_gpu(self.device)
        self.comm = comm if comm is not None else Comm()
        algo = args.get("algo", "happo")
        if algo not in ALGO_REGISTRY:
            raise NotImplementedError(f"algo {algo}: this round implements {sorted(ALGO_REGISTRY)}")
        self.num_agents = len(obs_spaces)
        self.state_type = (env_args or {}).get("state_type", "EP")
        if self.state_type not in ("EP", "FP"):
            raise ValueError(f"state_type {self.state_type}")
        self.share_param = bool(algo_args["algo"].get("share_param", False))
        if self.share_param and algo != "mappo":
            raise NotImplementedError("share_param is a MAPPO feature (HAPPO/HATRPO/HAA2C need per-agent actors)")
        self.fixed_order = algo_args["algo"].get("fixed_order", True)
        self.action_aggregation = algo_args["algo"]["action_aggregation"]
        if self.share_param and self.comm.world_size > 1 and (algo_args["model"].get("use_recurrent_policy")
                                                             or algo_args["model"].get("use_naive_recurrent_policy")):
            # refused before any rollout instead of in the first train() (configs.unsupported_reason has the why)
            raise NotImplementedError("share_param with recurrent policies under data parallelism is not implemented")

        n_global = algo_args["train"]["n_rollout_threads"]
        lo, hi = shard_columns(n_global, self.comm.rank, self.comm.world_size)
        self.n_global, self.col_lo, self.col_hi = n_global, lo, hi
        train_local = dict(algo_args["train"])
        train_local["n_rollout_threads"] = hi - lo
        margs = {**algo_args["model"], **algo_args["algo"]}
        self.actor: List[HAPPO] = []
        for a in range(self.num_agents):  # construction order = reference (actors 0..A-1, then critic) for RNG parity
            if self.share_param and a > 0:  # ONE actor object in every slot (on_policy_base_runner.py:96-113)
                self.actor.append(self.actor[0])
            else:
                self.actor.append(ALGO_REGISTRY[algo](margs, obs_spaces[a], act_spaces[a], device=self.device))
        self.actor_buffer = [OnPolicyActorBuffer({**train_local, **algo_args["model"]}, obs_spaces[a], act_spaces[a],
                                                 device=self.device) for a in range(self.num_agents)]
        self.critic = VCritic(margs, share_obs_space, device=self.device)
        cb_args = {**train_local, **algo_args["model"], **algo_args["algo"]}
        if self.state_type == "EP":
            self.critic_buffer = OnPolicyCriticBufferEP(cb_args, share_obs_space, device=self.device)
        else:
            self.critic_buffer = OnPolicyCriticBufferFP(cb_args, share_obs_space, self.num_agents, device=self.device)
        self.value_normalizer = ValueNorm(1, device=self.device) if algo_args["train"]["use_valuenorm"] else None
        self._critic_comm = self.comm.second_group()  # collective: every rank passes here, in constructor order
        self._init_update_state(n_global)
        if algo_args["train"].get("model_dir") is not None:  # on_policy_base_runner.py:168-169
            self.restore(algo_args["train"]["model_dir"])

    def _init_update_state(self, n_global: Optional[int] = None, comm: Optional[Comm] = None) -> None:
        """Everything train() / compute() need beyond the reference runner's own attributes (the drop-in subclasses of the
        reference's OnPolicyBaseRunner get it lazily through ``_ensure_update_state``): the communicator, this rank's column
        shard, and the pinned / device scratch of train()."""
        if not hasattr(self, "comm") or self.comm is None:
            self.comm = comm if comm is not None else Comm()
        if n_global is None:
            n_global = self.algo_args["train"]["n_rollout_threads"]
        if not hasattr(self, "col_lo"):
            self.n_global = n_global
            self.col_lo, self.col_hi = shard_columns(n_global, self.comm.rank, self.comm.world_size)
        shard = (self.n_global, self.col_lo, self.col_hi) if self.comm.enabled else None
        for x in list(self.actor) + [self.critic]:
            x.comm, x.shard = self.comm, shard
        for x in self.actor:  # (Gaussian heads of 33..64 dimensions are single-GPU: refused here, not in the first train())
            x._refuse_gauss_wide_dp()
        # HARL_CRITIC_GROUP=1: the critic's collectives go through a communicator of their own and its update keeps its own
        # stream under data parallelism.  The group is created by the constructors (collective call: never from this lazy
        # path, where ranks may arrive at different times); without one the critic shares the actors' communicator + stream.
        self.critic.comm = getattr(self, "_critic_comm", None) or self.comm
        self._logp_old = None
        self._counts_host = None
        self._update_state_ready = True

    def _ensure_update_state(self) -> None:
        if not getattr(self, "_update_state_ready", False):
            self._init_update_state()

    def _check_comms(self) -> None:
        """After train()'s read-back (the device is idle): a timed-out one-shot exchange has put NaNs into that step's
        gradients -- raise instead of training on.  No-op unless HARL_ALLREDUCE selected the one-shot path."""
        self.comm.check()
        if self.critic.comm is not self.comm:
            self.critic.comm.check()

    # ---- on_policy_base_runner.py:462-484 -------------------------------------------------------
    @torch.no_grad()
    def compute(self):
        self._ensure_update_state()
        cb = self.critic_buffer
        if self.state_type == "EP":
            next_value, _ = self.critic.get_values(cb.share_obs[-1], cb.rnn_states_critic[-1], cb.masks[-1])
        else:  # FP: all (thread, agent) rows in one batch (np.concatenate over threads, base_runner.py:472-481)
            so = cb.share_obs[-1]
            rows = so.shape[0] * so.shape[1]
            next_value, _ = self.critic.get_values(so.reshape(rows, -1), cb.rnn_states_critic[-1].reshape(rows, 1, -1),
                                                   cb.masks[-1].reshape(rows, 1))
        cb.compute_returns(next_value, self.value_normalizer)

    def _train_schedule(self, fast, B: int, on_gpu: bool) -> _TrainSchedule:
        """Where one train() call puts the critic's update and the actors' log-prob passes (``fast``: per actor, whether it
        has ``masked_moments``; ``B``: rows per minibatch of a full-buffer update; ``on_gpu``: the device is a GPU).  The only
        reader of the seven switches, at every call: bench.py and the tests flip them between the train() calls of one process.
        Everything here is known before the host waits for the active-entry counts.

        ``critic`` "first": the critic update may be enqueued before the actors'.  Only when nothing in train() materialises a
        permutation (one full-buffer minibatch everywhere, feed-forward nets, HAPPO-family actors): then every sampler merely
        advances the CPU generator by a count, the final generator state does not depend on the order of those advances, and the
        critic reads nothing the actors write.  Its kernels are enqueued BEFORE the host waits on the event behind the counts'
        copy: the GPU works through them while the host queues the first actor's launches instead of idling behind a drained
        stream.  HARL_CRITIC_FIRST=0: not first.
        ``critic_stream`` with "first": ... and on a stream of its own (single-GPU runs): the critic's twenty-odd launches are
        independent of the actors', and every one of these persistent kernels ends with a tail in which most CUs have run out of
        slabs (kernel time 0.19-0.26 ms against 0.14-0.20 ms for a wave's own slab loop, tools/phase_cycles.py) -- the other
        chain's next kernel fills it.  HARL_CRITIC_STREAM=0 keeps one stream.
        Under data parallelism the second stream needs the critic's own communicator (two chains issuing into ONE
        communicator would have to interleave their collectives identically on every rank).
        Round 6, session 3: ... and only where the launches are short.  From ~150 000 rows per minibatch every heavy kernel
        of either chain fills the chip for 0.2 - 0.5 ms (one workgroup per CU, LDS-bound occupancy): the other chain's light
        kernels then wait for a whole heavy launch to drain, the sum of the kernel times is the update either way, and
        one stream measured as fast or faster (16.06 against 16.18 ms at 4096 threads, 8.90 / 9.00 at 2048, 5.45 / 5.58 at
        1024 -- and 3.90 against 3.73 at 512 threads, where the second stream stays; profiles/r06s3_critic_stream_ab.md).
        HARL_CRITIC_STREAM=1 forces the second stream, 0 forbids it; any other value is the size rule.

        ``critic`` "staggered" (always on its own stream), round 6: the critic's update NEXT TO the actors' also where
        permutations are materialised (recurrent policies, several minibatches).  In the reference the critic's samplers draw from
        the global CPU generator AFTER every actor's, so the generator is fast-forwarded over the actors' draws first (their sizes
        are known: HAPPO.rng_footprint; agents without an active entry draw nothing, happo.py:119-120), the critic's train() -- on
        a stream of its own -- takes its permutations from exactly the state the reference's critic finds, and the generator goes
        back to where the actors start; at the end it is set to the state behind the critic's draws (_StaggeredCritic).  Every
        permutation and the final state are bit-identical to the in-order run.  What it buys: with GRU policies the main stream
        idles ~0.4 ms per agent behind the previous agent's post-update log-prob pass (a full-length chain on 6 % of the chip:
        3.9 of the SMAC update's 29.5 ms, rocprofv3 trace of round 6, profiles/r06_smac_timeline.md) and then ran the critic's
        2.4 ms at the very end; now the critic's launches fill those gaps.
        ... one EPOCH at a time (VCritic._train_epochs), epoch k enqueued right behind agent k's update and ordered behind
        its event: that is where the main stream goes idle (agent k + 1's loss waits for agent k's post-update pass); run
        all at once up front the critic only competed with the first agent's kernels (27.7 against 28.3 ms, SMAC 3s5z).
        HARL_CRITIC_STREAM=0 or HARL_CRITIC_EARLY=0: ``critic`` "last", after the actors on the main stream, the reference's order.

        ``side``: pre-update log-probs that cannot come out of the first epoch's forward (recurrent policies: full-length unroll
        from rnn_states[0]; several minibatches; which agents those are depends on the counts: train()'s ``fused_old``) depend
        only on the agent's OWN pre-update weights, not on the agents before it (on_policy_ha_runner.py:66-83) -- so they are
        enqueued on a side stream, where the long, narrow recurrences (N/32 dependent chains of T steps) run next to the update
        kernels of the agents in front instead of in series with them; agent k's update waits for event k.  HARL_SIDE_STREAM=0:
        on the main stream, in front of each agent's update.  (Not a question of the device: the tests' recorder on device "cpu"
        sets HARL_SIDE_STREAM=0.)
        ``side_ahead``: ... ONE AGENT AHEAD of the main stream (round 6, second session): enqueueing all of them up front is ~0.3
        ms of host time each -- the raw rocprofv3 trace of the 8-agent recurrent update showed the main queue EMPTY for the first
        2.6 of its 22.7 ms while the host was still feeding the side stream.  The first agent's pass goes out up front, agent
        k + 1's right behind the launches of agent k's update (2.5 ms of queued GPU work for a 0.47 ms pass): same kernels, same
        operands per agent.  HARL_SIDE_AHEAD=0: all up front, as before.

        ``post_stream``: post-update log-probs of RECURRENT policies (full-length unroll: N/32 dependent chains of T steps, ~0.5 ms
        on 32 waves of the chip at the SMAC sizes) go to a stream of their own when the next agent can await them: the next
        agent's first forward -- sequence tables, input image, MLP layers, the training GRU forward -- needs nothing from them;
        only its first LOSS launch consumes the factor and waits for the event (HAPPO._await_factor).  Same kernels, same
        operands, same order per tensor: bit-identical results.  HARL_POST_STREAM=0 keeps the pass on the main stream.
        ``last_post``: the factor behind the LAST agent of the order is handed to nobody (on_policy_ha_runner.py:96-124 computes
        it and drops it): no clone, no forward over the whole batch.  HARL_LAST_POST_PASS=1 runs it all the same (device "cpu"
        exists under the tests' launch recorder only, which pins the reference's one pass per agent)."""
        env = os.environ.get
        cs_mode = env("HARL_CRITIC_STREAM", "auto")
        own_comm = not self.comm.enabled or self.critic.comm is not self.comm
        if (all(fast) and env("HARL_CRITIC_FIRST", "1") != "0" and self.critic.one_full_minibatch()
                and all(hasattr(a, "fuses_old_logp") and a.fuses_old_logp() for a in self.actor)):
            critic, critic_stream = "first", bool(on_gpu and own_comm and cs_mode != "0"
                                                  and (cs_mode == "1" or B <= self.CRITIC_STREAM_MAX_ROWS))
        elif (on_gpu and all(hasattr(a, "rng_footprint") for a in self.actor) and own_comm
              and cs_mode != "0" and env("HARL_CRITIC_EARLY", "1") != "0"):
            critic, critic_stream = "staggered", True
        else:
            critic, critic_stream = "last", False
        return _TrainSchedule(critic, critic_stream, side=env("HARL_SIDE_STREAM", "1") != "0",
                              side_ahead=env("HARL_SIDE_AHEAD", "1") != "0",
                              post_stream=on_gpu and env("HARL_POST_STREAM", "1") != "0",
                              last_post=env("HARL_LAST_POST_PASS", "0") == "1" or not on_gpu)

    # ---- on_policy_ha_runner.py:11-130 ------------------------------------------------------------
    @torch.no_grad()
    def train(self):
        self._ensure_update_state()
        T = self.algo_args["train"]["episode_length"]
        N = self.col_hi - self.col_lo
        B = T * N
        dev = self.device
        on_gpu = dev.type == "cuda"
        main = torch.cuda.current_stream(dev) if on_gpu else None
        actor_train_infos = []
        for x in self.actor:  # cached normalised-input images never outlive one update (nets.invalidate_caches)
            x.actor.invalidate_caches()
        self._prepare_inputs()
        factor = torch.ones(T, N, 1, dtype=torch.float32, device=dev)
        advantages = self.critic_buffer.advantages  # returns[:-1] - denormalize(value_preds[:-1]), fused into the GAE scan
        if self.state_type == "FP":
            advantages = self._fp_normalised_advantages(advantages)
        if self.fixed_order:
            agent_order = list(range(self.num_agents))
        else:
            rng_sync()
            agent_order = [int(a) for a in torch.randperm(self.num_agents).numpy()]  # first CPU-RNG draw of train()
        # ---- moments.  Host syncs per train(): ONE read-back of every agent's active-entry count up front (early-out test,
        # happo.py:119-120) and ONE of all training statistics at the end; nothing in between waits for the GPU.
        fast = [hasattr(a, "masked_moments") for a in self.actor]
        mom_all = torch.zeros(self.num_agents, 3, dtype=torch.float64, device=dev)
        for a in range(self.num_agents):
            if fast[a]:
                adv_a = advantages if self.state_type == "EP" else advantages[:, :, a].contiguous()
                self.actor[a].masked_moments(self.actor_buffer[a], adv_a, mom_all[a])
        self.comm.all_reduce_sum(mom_all)
        # The only mid-train host read: the active-entry counts, an asynchronous copy into pinned memory followed by an event
        if self._counts_host is None or self._counts_host.numel() != self.num_agents:
            self._counts_host = torch.empty(self.num_agents, dtype=torch.float64, pin_memory=torch.cuda.is_available())
        self._counts_host.copy_(mom_all[:, 2], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        # ---- schedule, and the critic's update where it goes first: before the host waits for the counts
        sched = self._train_schedule(fast, B, on_gpu)
        cs, cinfo, critic_done, stagger = None, None, None, None
        if sched.critic == "first":
            if sched.critic_stream:
                cs = _stream(self, "_critic_stream")
                cs.wait_stream(main)
            with _on(cs):
                cinfo = self.critic.train(self.critic_buffer, self.value_normalizer, _defer=True)
                if cs is not None:
                    critic_done = torch.cuda.Event()
                    critic_done.record(cs)
        # ---- counts, and the two facts per agent that depend on them: whether its pre-update log-probs come out of its first
        # forward (with one full-buffer minibatch the first epoch's forward inside train() computes exactly these: same rows,
        # same parameters), and whether it draws from the generator at all (the staggered critic's footprint)
        ev.synchronize()
        counts = self._counts_host.tolist()
        fused_old = [fast[a] and self.actor[a].fuses_old_logp() and counts[a] > 0.0 for a in range(self.num_agents)]
        if sched.critic == "staggered":
            footprint = [n for a in agent_order if counts[a] > 0.0 for n in self.actor[a].rng_footprint(self.actor_buffer[a])]
            cs = _stream(self, "_critic_stream")
            cs.wait_stream(main)
            stagger = _StaggeredCritic(self.critic._train_epochs(self.critic_buffer, self.value_normalizer),
                                       self.critic.critic_epoch, footprint, cs)
        # ---- the side stream
        passes, old_all, old_ev = {}, {}, {}

        def logp_inputs(a):
            """((obs, actions, available actions, B), recurrent keywords) of agent a's log-prob passes, built once.  Its weights
            are folded first, on the stream that is current, at every call: free when nothing has touched them since."""
            act_a, buf_a = self.actor[a], self.actor_buffer[a]
            act_a.actor.fold()
            if a not in passes:
                kw_a = dict(rnn_states=buf_a.rnn_states[0], masks=buf_a.flat("masks")) if act_a.actor.recurrent else {}
                avail = None if buf_a.available_actions is None else buf_a.flat("available_actions")
                passes[a] = ((buf_a.flat("obs"), buf_a.flat("actions"), avail, B), kw_a)
            return passes[a]

        def enqueue_old_logp(a):
            """Agent a's pre-update pass on the side stream (+ the event its update waits for)."""
            with torch.cuda.stream(self._side_stream):
                args_a, kw_a = logp_inputs(a)
                self.actor[a]._logp_pass(*args_a, old_all[a], **kw_a)
                old_ev[a] = torch.cuda.Event()
                old_ev[a].record(self._side_stream)

        side_pending = [a for a in agent_order if not fused_old[a]] if sched.side else []
        if side_pending:
            _stream(self, "_side_stream").wait_stream(main)
            for a in side_pending:
                old_all[a] = torch.empty(B, self.actor[a].actor.act_w, dtype=torch.float32, device=dev)
            for _ in range(1 if sched.side_ahead else len(side_pending)):
                enqueue_old_logp(side_pending.pop(0))
        # ---- the agents, in order
        pending, keep_alive = [], []
        factor_ev, prev_overlapped = None, False
        for pos, agent_id in enumerate(agent_order):
            buf, actor = self.actor_buffer[agent_id], self.actor[agent_id]
            if agent_id in old_ev:  # this agent's networks / workspaces are in use on the side stream until then
                main.wait_event(old_ev[agent_id])
            buf.update_factor(factor)
            if prev_overlapped:  # the post stream still reads the previous agent's pre-update log-probs: do not write into them
                keep_alive.append(self._logp_old)
                self._logp_old = None
            if self._logp_old is None or self._logp_old.shape != (B, actor.actor.act_w):
                self._logp_old = torch.empty(B, actor.actor.act_w, dtype=torch.float32, device=dev)
            logp_args, rnn_kw = logp_inputs(agent_id)
            adv_a = advantages if self.state_type == "EP" else advantages[:, :, agent_id].contiguous()
            kw = dict(_pre=(mom_all[agent_id], counts[agent_id]), _defer=True) if fast[agent_id] else {}
            if fused_old[agent_id]:  # pre-update log-probs (:66-83): out of the first forward, off the side stream, or here
                kw["_old_logp_out"] = self._logp_old
            elif agent_id in old_all:
                self._logp_old = old_all.pop(agent_id)
            else:
                actor._logp_pass(*logp_args, self._logp_old, **rnn_kw)
            if factor_ev is not None and hasattr(actor, "_factor_ready"):
                actor._factor_ready = factor_ev
            info = actor.train(buf, adv_a, self.state_type, **kw)               # :86-93
            if side_pending:  # the next agent's pre-update pass, behind this agent's queued launches (``side_ahead``)
                enqueue_old_logp(side_pending.pop(0))
            if stagger is not None and stagger.left > 0:  # one critic epoch behind this agent's optimiser steps
                ev_a = torch.cuda.Event()
                ev_a.record(main)
                stagger.epoch(ev_a)
            if factor_ev is not None:  # (an update that never reached a loss launch has not waited yet)
                if hasattr(actor, "_factor_ready"):
                    actor._factor_ready = None
                main.wait_event(factor_ev)
                factor_ev = None
            pending.append((len(actor_train_infos), info, actor._INFO_KEYS) if torch.is_tensor(info) else None)
            actor_train_infos.append(info)
            nxt = agent_order[pos + 1] if pos + 1 < len(agent_order) else None
            prev_overlapped = bool(sched.post_stream and nxt is not None and actor.actor.recurrent
                                   and hasattr(self.actor[nxt], "_factor_ready"))
            if nxt is None and not sched.last_post:
                continue
            ps = _stream(self, "_post_stream") if prev_overlapped else None
            if ps is not None:
                ps.wait_stream(main)  # this agent's optimiser steps are complete
                keep_alive += [factor, self._logp_old]
            with _on(ps):
                new_factor = factor.clone()
                # post-update log-probs fused with factor *= agg(exp(new - old))   (:96-124)
                actor._logp_pass(*logp_args, None, old_logp=self._logp_old, factor=new_factor.reshape(B), **rnn_kw)
                if ps is not None:
                    factor_ev = torch.cuda.Event()
                    factor_ev.record(ps)
            factor = new_factor
        # ---- close
        if keep_alive:  # tensors of the main stream's allocator pool that the post stream has read
            main.wait_stream(self._post_stream)
            keep_alive.clear()
        if stagger is not None:  # epochs not handed out yet (fewer agents than critic epochs), then the critic's statistics
            stagger.finish()
            with torch.cuda.stream(cs):
                cinfo = self.critic._train_result(True)
                critic_done = torch.cuda.Event()
                critic_done.record(cs)
        if cinfo is None:
            cinfo = self.critic.train(self.critic_buffer, self.value_normalizer, _defer=True)
        if critic_done is not None:
            main.wait_event(critic_done)
        rng_sync()  # the global CPU generator is exactly where the reference leaves it
        if stagger is not None:  # ... i.e. behind the critic's draws, which were taken from their own position
            torch.set_rng_state(stagger.state)
        dev_infos = [p[1] for p in pending if p is not None] + [cinfo]
        flat = torch.cat([t.reshape(-1) for t in dev_infos]).cpu().tolist()  # the single end-of-train read-back
        self._check_comms()
        off = 0
        for p in pending:
            if p is not None:
                i, _, keys = p
                actor_train_infos[i] = dict(zip(keys, flat[off:off + len(keys)]))
                off += len(keys)
        critic_train_info = {"value_loss": flat[off], "critic_grad_norm": flat[off + 1]}
        return actor_train_infos, critic_train_info

    def _prepare_inputs(self) -> None:
        """Head of train(): every feed-forward network's folded weights (one harl_fold_table each) and then ALL their
        normalised-input images in ONE launch (nets.prepare_x0n_multi), enqueued back to back before the first agent's
        update.  Lazily, each network built its image where its update first read it, a latency-bound launch behind the host
        work at the head of that update (0.19 ms of idle GPU in front of the critic's, profiles/r06s3_kernel_trace_mpe.md).
        Neither depends on anything train() computes: a network's parameters change in its own update only, the observation
        buffers not at all.  Same kernels' arithmetic, same operands: bit-identical.  The critic's entry invalidation happens
        here instead of in VCritic._train_epochs (told through ``_inputs_prepared``), so its image lives for this train() as
        before.  Networks that are not covered -- recurrent, several minibatches (gathered rows), inputs wider than 64, an
        empty data-parallel shard, HARL_GRAPH=1 -- keep the lazy launches; HARL_X0N_MULTI=0 keeps them everywhere."""
        from . import graphs
        if os.environ.get("HARL_X0N_MULTI", "1") == "0" or self.device.type != "cuda" or graphs.enabled():
            return
        from .nets import prepare_x0n_multi
        items = []
        for a, buf in zip(self.actor, self.actor_buffer):
            if hasattr(a, "fuses_old_logp") and a.fuses_old_logp():
                items.append((a.actor, buf.flat("obs")))
        c = self.critic
        crit = hasattr(c, "_inputs_prepared") and c.one_full_minibatch()
        if crit:
            c.critic.invalidate_caches()
            items.append((c.critic, self.critic_buffer.flat("share_obs")))
        for net, _ in items:
            net.fold()
        built = prepare_x0n_multi([(net, X, X.shape[0]) for net, X in items])
        if crit and built:
            c._inputs_prepared = True  # (consumed by the critic's train(): it does not invalidate again)

    def graph_stats(self) -> dict:
        """Sum of the actors' and the critic's ``graph_stats()`` (HARL_GRAPH=1: captured / replayed / eager optimiser steps)."""
        from .graphs import sum_stats
        return sum_stats(list(self.actor) + [self.critic])

    def after_update(self):
        for b in self.actor_buffer:
            b.after_update()
        self.critic_buffer.after_update()

    def _fp_normalised_advantages(self, advantages):
        """Global masked normalisation over every agent's active entries (on_policy_ha_runner.py:36-45,
        on_policy_ma_runner.py:25-36)."""
        dev = self.device
        active = torch.stack([b.active_masks[:-1] for b in self.actor_buffer], dim=2).contiguous()  # [T,N,A,1]
        mom = torch.zeros(3, dtype=torch.float64, device=dev)
        n = advantages.numel()
        call("harl_masked_moments", ptr(advantages), ptr(active), n, ptr(mom), _lib.scratch("mm"), stream())
        self.comm.all_reduce_sum(mom)
        adv_n = torch.empty_like(advantages)
        call("harl_adv_normalize", ptr(advantages), ptr(mom), ptr(adv_n), n, stream())
        return adv_n

    # ---- rollout side (on_policy_base_runner.py:171-460): the loop is the reference's; what changes is where the data
    # lives.  Observations go up once per step, actions come down once per step; log-probs, values, hidden states, masks
    # and everything the update reads never leave the device.
    def warmup(self):
        """Reset the environments and fill slot 0 of the buffers (on_policy_base_runner.py:269-283)."""
        obs, share_obs, available_actions = self.envs.reset()
        obs = torch.as_tensor(obs, dtype=torch.float32).to(self.device)
        for a in range(self.num_agents):
            self.actor_buffer[a].obs[0].copy_(obs[:, a])
            if self.actor_buffer[a].available_actions is not None:
                av = torch.as_tensor(available_actions, dtype=torch.float32).to(self.device)
                self.actor_buffer[a].available_actions[0].copy_(av[:, a])
        so = torch.as_tensor(share_obs, dtype=torch.float32).to(self.device)
        self.critic_buffer.share_obs[0].copy_(so[:, 0] if self.state_type == "EP" else so)

    @torch.no_grad()
    def collect(self, step: int):
        """Sample actions from every actor and values from the critic at buffer slot ``step`` (:285-343).  Returns DEVICE
        tensors (values [N,1] | [N,A,1], actions [N,A,act_w], action_log_probs, rnn_states [N,A,1,H],
        rnn_states_critic [N,1,H] | [N,A,1,H])."""
        acts, logps, rnns = [], [], []
        for a in range(self.num_agents):
            b = self.actor_buffer[a]
            action, logp, rnn = self.actor[a].get_actions(
                b.obs[step], b.rnn_states[step], b.masks[step],
                b.available_actions[step] if b.available_actions is not None else None)
            acts.append(action)
            logps.append(logp)
            rnns.append(rnn.reshape(rnn.shape[0], b.recurrent_n, -1))
        actions, action_log_probs, rnn_states = torch.stack(acts, 1), torch.stack(logps, 1), torch.stack(rnns, 1)
        cb = self.critic_buffer
        if self.state_type == "EP":
            values, rnn_c = self.critic.get_values(cb.share_obs[step], cb.rnn_states_critic[step], cb.masks[step])
            rnn_c = rnn_c.reshape(values.shape[0], cb.recurrent_n, -1)
        else:
            so = cb.share_obs[step]
            N, A = so.shape[:2]
            values, rnn_c = self.critic.get_values(so.reshape(N * A, -1), cb.rnn_states_critic[step].reshape(N * A, 1, -1),
                                                   cb.masks[step].reshape(N * A, 1))
            values, rnn_c = values.reshape(N, A, 1), rnn_c.reshape(N, A, cb.recurrent_n, -1)
        return values, actions, action_log_probs, rnn_states, rnn_c

    @torch.no_grad()
    def insert(self, data):
        """Write one environment step into the buffers (:345-460): hidden states reset and masks 0 where the whole
        environment is done, active_masks 0 for agents that died, bad_masks 0 on truncation (``bad_transition``)."""
        (obs, share_obs, rewards, dones, infos, available_actions, values, actions, action_log_probs, rnn_states,
         rnn_states_critic) = data
        dev, A = self.device, self.num_agents
        up = lambda x: torch.as_tensor(x, dtype=torch.float32).to(dev)  # noqa: E731
        dones = torch.as_tensor(dones).to(dev).bool()
        N = dones.shape[0]
        dones_env = dones.all(dim=1)
        keep = (~dones_env).to(torch.float32)
        rnn_states = rnn_states * keep.view(N, 1, 1, 1)
        rnn_states_critic = rnn_states_critic * (keep.view(N, 1, 1) if self.state_type == "EP" else keep.view(N, 1, 1, 1))
        masks = keep.view(N, 1, 1).expand(N, A, 1)
        active_masks = torch.where(dones & ~dones_env.view(N, 1), 0.0, 1.0).view(N, A, 1)
        if self.state_type == "EP":
            bad = [[0.0] if info[0].get("bad_transition", False) is True else [1.0] for info in infos]
        else:
            bad = [[[0.0] if info[a].get("bad_transition", False) is True else [1.0] for a in range(A)] for info in infos]
        bad_masks = torch.tensor(bad, dtype=torch.float32, device=dev)
        obs, rewards, share_obs = up(obs), up(rewards), up(share_obs)
        avail = None if (available_actions is None or available_actions[0] is None) else up(available_actions)
        for a in range(A):
            self.actor_buffer[a].insert(obs[:, a], rnn_states[:, a], actions[:, a], action_log_probs[:, a], masks[:, a],
                                        active_masks[:, a], None if avail is None else avail[:, a])
        if self.state_type == "EP":
            self.critic_buffer.insert(share_obs[:, 0], rnn_states_critic, values, rewards[:, 0], masks[:, 0], bad_masks)
        else:
            self.critic_buffer.insert(share_obs, rnn_states_critic, values, rewards, masks, bad_masks)

    def run(self, num_episodes: Optional[int] = None):
        """The reference's training loop (:171-267) over ``self.envs``: warmup, then per episode lr decay, T x
        (collect -> envs.step -> insert), compute, train, [log], every ``eval_interval`` episodes [eval +] save,
        after_update.  Returns the per-episode (actor_train_infos, critic_train_info, mean step reward) list; ``logger``
        callbacks are invoked if one was given; checkpoints go to ``self.save_dir`` when it is set."""
        if self.envs is None:
            raise RuntimeError("run() needs a vectorised environment (envs=...)")
        tr = self.algo_args["train"]
        T = tr["episode_length"]
        episodes = num_episodes if num_episodes is not None else int(tr["num_env_steps"]) // T // tr["n_rollout_threads"]
        self.warmup()
        if self.logger is not None:
            self.logger.init(episodes)
        history = []
        for episode in range(1, episodes + 1):
            if tr.get("use_linear_lr_decay", False):
                for a in self.actor:
                    a.lr_decay(episode, episodes)
                self.critic.lr_decay(episode, episodes)
            if self.logger is not None:
                self.logger.episode_init(episode)
            self.prep_rollout()
            for step in range(T):
                values, actions, logp, rnn, rnn_c = self.collect(step)
                obs, share_obs, rewards, dones, infos, avail = self.envs.step(actions.cpu().numpy())
                data = (obs, share_obs, rewards, dones, infos, avail, values, actions, logp, rnn, rnn_c)
                if self.logger is not None:
                    self.logger.per_step(data)
                self.insert(data)
            self.compute()
            self.prep_training()
            infos_a, info_c = self.train()
            history.append((infos_a, info_c, self.critic_buffer.get_mean_rewards()))
            if self.logger is not None and episode % tr.get("log_interval", 1) == 0:
                self.logger.episode_log(infos_a, info_c, self.actor_buffer, self.critic_buffer)
            if episode % tr.get("eval_interval", 25) == 0:  # on_policy_base_runner.py:252-258
                if self.algo_args.get("eval", {}).get("use_eval", False) and self.eval_envs is not None:
                    self.prep_rollout()
                    self.eval()
                if getattr(self, "save_dir", None):
                    self.save(self.save_dir)
            self.after_update()
        return history

    @torch.no_grad()
    def eval(self):
        """Deterministic evaluation episodes on ``self.eval_envs`` (on_policy_base_runner.py:499-590): actions from
        ``actor.act(..., deterministic=True)``, hidden states reset and masks 0 where an environment finished, logger
        callbacks ``eval_init / eval_per_step / eval_thread_done / eval_log``; returns the mean episode reward."""
        import numpy as np
        ev = self.algo_args["eval"]
        n_thr, A = ev["n_eval_rollout_threads"], self.num_agents
        lg = self.logger
        if lg is not None:
            lg.eval_init()
        obs, _share, avail = self.eval_envs.reset()
        H = self.algo_args["model"]["hidden_sizes"][-1]
        rn = self.algo_args["model"]["recurrent_n"]
        rnn = torch.zeros(n_thr, A, rn, H, dtype=torch.float32, device=self.device)
        masks = torch.ones(n_thr, A, 1, dtype=torch.float32, device=self.device)
        done_eps, ep_rewards, cur = 0, [], np.zeros(n_thr)
        while True:
            acts = []
            obs_d = torch.as_tensor(np.asarray(obs), dtype=torch.float32).to(self.device)
            av_d = None if (avail is None or avail[0] is None) else torch.as_tensor(np.asarray(avail), dtype=torch.float32).to(self.device)
            for a in range(A):
                act, r_ = self.actor[a].act(obs_d[:, a], rnn[:, a], masks[:, a], None if av_d is None else av_d[:, a],
                                            deterministic=True)
                rnn[:, a] = r_.reshape(n_thr, rn, H)
                acts.append(act)
            actions = torch.stack(acts, 1).cpu().numpy()
            obs, share, rewards, dones, infos, avail = self.eval_envs.step(actions)
            if lg is not None:
                lg.eval_per_step((obs, share, rewards, dones, infos, avail))
            cur += np.mean(np.asarray(rewards), axis=1).reshape(n_thr)
            dones_env = np.all(np.asarray(dones), axis=1)
            keep = torch.as_tensor(~dones_env).to(self.device).float()
            rnn = rnn * keep.view(n_thr, 1, 1, 1)
            masks = keep.view(n_thr, 1, 1).expand(n_thr, A, 1).contiguous()
            for i in range(n_thr):
                if dones_env[i]:
                    done_eps += 1
                    ep_rewards.append(cur[i])
                    cur[i] = 0.0
                    if lg is not None:
                        lg.eval_thread_done(i)
            if done_eps >= ev["eval_episodes"]:
                if lg is not None:
                    lg.eval_log(done_eps)
                return float(np.mean(ep_rewards))

    @torch.no_grad()
    def render(self, expand_dims: bool = False, manual_render: bool = False, delay: float = 0.0) -> List[float]:
        """Roll the deterministic policy through ``algo_args['render']['render_episodes']`` episodes of ``self.envs``
        (on_policy_base_runner.py:594-710).  ``expand_dims``: the environment is a single instance without the parallel-
        environment axis (the reference's ``manual_expand_dims`` environments); ``manual_render`` calls ``envs.render()``
        after every step, ``delay`` sleeps between steps.  Returns the episode returns (the reference prints them)."""
        import time

        import numpy as np
        A = self.num_agents
        H = self.algo_args["model"]["hidden_sizes"][-1]
        rn = self.algo_args["model"]["recurrent_n"]
        returns = []
        for _ in range(self.algo_args["render"]["render_episodes"]):
            obs, _share, avail = self.envs.reset()
            n = 1 if expand_dims else len(obs)
            rnn = torch.zeros(n, A, rn, H, dtype=torch.float32, device=self.device)
            masks = torch.ones(n, A, 1, dtype=torch.float32, device=self.device)
            total = 0.0
            while True:
                obs_d = torch.as_tensor(np.asarray(obs), dtype=torch.float32).to(self.device).reshape(n, A, -1)
                no_av = avail is None or (not expand_dims and avail[0] is None)
                av_d = None if no_av else torch.as_tensor(np.asarray(avail), dtype=torch.float32).to(self.device).reshape(n, A, -1)
                acts = []
                for a in range(A):
                    act, r_ = self.actor[a].act(obs_d[:, a], rnn[:, a], masks[:, a], None if av_d is None else av_d[:, a],
                                                deterministic=True)
                    rnn[:, a] = r_.reshape(n, rn, H)
                    acts.append(act)
                actions = torch.stack(acts, 1).cpu().numpy()
                obs, _share, rewards, dones, _infos, avail = self.envs.step(actions[0] if expand_dims else actions)
                r0, d0 = np.asarray(rewards), np.asarray(dones)
                total += float(r0.reshape(-1)[0])
                if manual_render:
                    self.envs.render()
                if delay > 0.0:
                    time.sleep(delay)
                if bool(d0.reshape(-1)[0]):
                    print(f"total reward of this episode: {total}")
                    returns.append(total)
                    break
        return returns

    def close(self):
        for e in (self.envs, getattr(self, "eval_envs", None)):
            if e is not None and hasattr(e, "close"):
                e.close()

    def prep_rollout(self):
        for a in self.actor:
            a.prep_rollout()
        self.critic.prep_rollout()

    def prep_training(self):
        for a in self.actor:
            a.prep_training()
        self.critic.prep_training()

    # ---- on_policy_base_runner.py:724-763: same file names, same state_dict keys ---------------------
    def save(self, save_dir: Optional[str] = None):
        if save_dir is None:
            save_dir = self.save_dir
        save_dir = str(save_dir)
        os.makedirs(save_dir, exist_ok=True)
        for a in range(self.num_agents):
            torch.save(self.actor[a].actor.state_dict(), os.path.join(save_dir, f"actor_agent{a}.pt"))
        torch.save(self.critic.critic.state_dict(), os.path.join(save_dir, "critic_agent.pt"))
        if self.value_normalizer is not None:
            torch.save(self.value_normalizer.state_dict(), os.path.join(save_dir, "value_normalizer.pt"))

    def restore(self, model_dir: Optional[str] = None):
        if model_dir is None:
            model_dir = self.algo_args["train"]["model_dir"]
        for a in range(self.num_agents):
            self.actor[a].actor.load_state_dict(torch.load(os.path.join(model_dir, f"actor_agent{a}.pt"), map_location=self.device))
        self.critic.critic.load_state_dict(torch.load(os.path.join(model_dir, "critic_agent.pt"), map_location=self.device))
        p = os.path.join(model_dir, "value_normalizer.pt")
        if self.value_normalizer is not None and os.path.exists(p):
            self.value_normalizer.load_state_dict(torch.load(p, map_location=self.device))


class OnPolicyMARunner(OnPolicyHARunner):
    """MAPPO: simultaneous (not sequential) actor updates without the factor (runners/on_policy_ma_runner.py:10-64),
    optionally with ONE parameter-shared actor."""

    @torch.no_grad()
    def train(self):
        self._ensure_update_state()
        dev = self.device
        A = self.num_agents
        for x in self.actor:
            x.actor.invalidate_caches()
        advantages = self.critic_buffer.advantages
        if self.state_type == "FP":
            advantages = self._fp_normalised_advantages(advantages)
        mom_all = torch.zeros(A, 3, dtype=torch.float64, device=dev)
        for a in range(A):
            adv_a = advantages if self.state_type == "EP" else advantages[:, :, a].contiguous()
            self.actor[a].masked_moments(self.actor_buffer[a], adv_a, mom_all[a])
        self.comm.all_reduce_sum(mom_all)
        dev_infos = []
        if self.share_param:
            info = self.actor[0].share_param_train(self.actor_buffer, advantages, A, self.state_type,
                                                   _moments=mom_all.sum(0), _defer=True)
            rng_sync()
            torch.randperm(A)  # on_policy_ma_runner.py:42-43 iterates over a fresh permutation: one more CPU-RNG draw
            dev_infos = [info]
            slots = [0] * A
        else:
            counts = mom_all[:, 2].cpu().tolist()
            slots = []
            for a in range(A):
                buf = self.actor_buffer[a]
                buf.factor = None
                adv_a = advantages if self.state_type == "EP" else advantages[:, :, a].contiguous()
                info = self.actor[a].train(buf, adv_a, self.state_type, _pre=(mom_all[a], counts[a]), _defer=True)
                if torch.is_tensor(info):
                    slots.append(len(dev_infos))
                    dev_infos.append(info)
                else:
                    slots.append(info)  # early-out dict (no active entries)
        cinfo = self.critic.train(self.critic_buffer, self.value_normalizer, _defer=True)
        rng_sync()
        flat = torch.cat([t.reshape(-1) for t in dev_infos] + [cinfo.reshape(-1)]).cpu().tolist()
        self._check_comms()
        keys = self.actor[0]._INFO_KEYS
        actor_train_infos = [s if isinstance(s, dict) else dict(zip(keys, flat[4 * s:4 * s + 4])) for s in slots]
        off = 4 * len(dev_infos)
        return actor_train_infos, {"value_loss": flat[off], "critic_grad_norm": flat[off + 1]}


RUNNER_REGISTRY = {"happo": OnPolicyHARunner, "hatrpo": OnPolicyHARunner, "haa2c": OnPolicyHARunner,
                   "mappo": OnPolicyMARunner}
