"""HAPPO on MI355X: same class surface as the reference (harl/algorithms/actors/on_policy_base.py:8-137,
harl/algorithms/actors/happo.py:10-158), arithmetic in libharl_hip.so.

One ``update`` = fold -> trunk forward (MFMA) -> fused head/loss/backward-to-dz_L -> weight-gradient partials
(MFMA) -> deterministic reduce + unfold -> [data-parallel all-reduce] -> fused grad-norm/clip/Adam.  Nothing
returns to the host inside ``train()`` except the int64 minibatch permutations going up and one small read-back
of the accumulated training statistics at the end.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib, graphs
from ._lib import PS_STRIDE, call, ptr, stream
from .buffers import OnPolicyActorBuffer, consume_randperm, minibatch_indices, rng_sync
from .configs import GAUSS_WIDE_REFUSALS
from .dist import Comm, local_minibatch_rows
from .nets import FusedAdam, StochasticPolicy, build_seq, routing_switches, seq_compact
from .valuenorm import _as_dev


class OnPolicyBase:
    """Actor + optimiser (reference: actors/on_policy_base.py:8-137)."""

    def __init__(self, args, obs_space, act_space, device=torch.device("cuda:0")):
        self.args = args
        self.device = torch.device(device)
        _lib.require_gpu(self.device)
        self.tpdv = dict(dtype=torch.float32, device=self.device)
        self.data_chunk_length = args["data_chunk_length"]
        self.use_recurrent_policy = args["use_recurrent_policy"]
        self.use_naive_recurrent_policy = args["use_naive_recurrent_policy"]
        self.use_policy_active_masks = args["use_policy_active_masks"]
        self.action_aggregation = args["action_aggregation"]
        self.lr = args["lr"]
        self.opti_eps = args["opti_eps"]
        self.weight_decay = args["weight_decay"]
        self.obs_space = obs_space
        self.act_space = act_space
        self.actor = StochasticPolicy(args, obs_space, act_space, self.device)
        self.actor_optimizer = FusedAdam(self.actor, self.lr, self.opti_eps, self.weight_decay)
        self.comm = Comm()
        self.shard = None  # (n_global, lo, hi) when n_rollout_threads is sharded across ranks
        self._refuse_gauss_wide_dp()
        self._old_logp: Optional[torch.Tensor] = None
        self._graph = graphs.GraphedStep("the actor")  # HARL_GRAPH=1: captured optimiser steps (HAPPO / HAA2C / MAPPO)
        self._graph_bufs: dict = {}   # persistent copies of what arrives as a fresh tensor per train()
        self._graph_gen = None

    def graph_stats(self) -> dict:
        """dict(captures, replays, eager_steps) of this actor's optimiser steps under HARL_GRAPH=1 (all zero without it)."""
        return self._graph.stats()

    def _refuse_gauss_wide_dp(self) -> None:
        """Gaussian heads of 33..64 dimensions: their log_std sums (net.ls_sum) are not part of the data-parallel message."""
        if self.actor.gauss_wide and (self.comm.enabled or self.shard is not None):
            raise NotImplementedError(GAUSS_WIDE_REFUSALS["dp"])

    def _graph_config_ok(self) -> bool:
        """HARL_GRAPH=1 and a configuration whose optimiser steps may be replayed from a hipGraph: feed-forward, one action
        head (Gaussian / Categorical of up to 64 actions), no data parallelism.  Everything else stays eager, exactly as without
        the variable."""
        return (graphs.enabled() and not (self.use_recurrent_policy or self.use_naive_recurrent_policy)
                and not self.actor.recurrent and not self.actor.grouped and not self.actor.gauss_wide
                and not self.comm.enabled and self.shard is None)

    def _graph_stage(self, name: str, t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """Copy ``t`` into this actor's persistent buffer ``name`` (a captured step holds ADDRESSES)."""
        if t is None:
            return None
        b = self._graph_bufs.get(name)
        if b is None or b.shape != t.shape or b.dtype != t.dtype or b.device != t.device:
            b = self._graph_bufs[name] = torch.empty_like(t, memory_format=torch.contiguous_format)
        b.copy_(t)
        return b

    def lr_decay(self, episode, episodes):  # utils/models_tools.py:77-87
        lr = self.lr - (self.lr * ((episode - 1) / float(episodes)))
        for g in self.actor_optimizer.param_groups:
            g["lr"] = lr

    # ---- log-prob passes over a whole [T*N] batch (on_policy_ha_runner.py:66-83,96-113) --------------
    def _logp_pass(self, obs, actions, avail, M, logp_out, old_logp=None, factor=None, head_out=None,
                   rnn_states=None, masks=None, h_last=False, reuse_trunk=False):
        """Forward + head over rows 0..M-1.  Recurrent nets follow the reference's convention (rnn.py:24-42): with
        rnn_states [m, 1, H], M = L*m rows are L steps of m sequences (l-major) unrolled from rnn_states with mask
        resets.  Returns the final hidden state [m, H] when ``h_last`` is set."""
        net = self.actor
        agg = int(self.action_aggregation == "mean")
        if not reuse_trunk and net._step_route(True, True, train=False).kind == "fused":  # forward + head in one launch, x_hat_2 never leaves the chip
            call("harl_update_logp", *net.fused_args(obs, M), *net.dist_args(), ptr(actions), ptr(avail), ptr(logp_out),
                 ptr(old_logp), ptr(factor), agg, ptr(head_out), stream(), tag="update_logp")
            return None
        if not net.recurrent:
            if not reuse_trunk:  # reuse_trunk: x_hat_L of these rows under the current weights is still in the workspace
                net.forward_trunk(obs, None, M, for_backward=False)
            net.head_logp(M, actions, avail, logp_out, old_logp, factor, head_out, agg)
            return None
        H = net.hidden_sizes[-1]
        m = rnn_states.shape[0]
        L = M // m
        HS = H * net.recurrent_n  # state row: the layers' hidden vectors side by side (rnn_states [m, recurrent_n, H])
        seq = build_seq(self.device, L, m, HS, h0=_as_dev(rnn_states, self.device).reshape(m, HS),
                        masks_src=_as_dev(masks, self.device), want_h_last=h_last)
        idx, Mp = seq["idx"], L * seq["m_pad"]
        padded = idx is not None
        g = (lambda t: None if t is None else t[idx].contiguous()) if padded else (lambda t: t)  # noqa: E731
        tmp = (lambda t: None if t is None else torch.empty(Mp, *t.shape[1:], **self.tpdv)) if padded else (lambda t: t)  # noqa: E731
        a_p, av_p, old_p, f_p = g(actions), g(avail), g(old_logp), g(factor)
        lo_p, ho_p = tmp(logp_out), tmp(head_out)
        net.forward_trunk(obs, idx, Mp, for_backward=False, seq=seq)
        net.head_logp(Mp, a_p, av_p, lo_p, old_p, f_p, ho_p, agg, m, seq["m_pad"])
        if padded:
            for dst, src in ((logp_out, lo_p), (head_out, ho_p), (factor, f_p)):
                if dst is not None:
                    dst.copy_(seq_compact(src, seq))
        return None if not h_last else seq["h_last"][:m]

    def _dist_rows(self, head, M, *, noise=None, actions=None, logp=None, probs=None, argmax_out=None, ent_rows=None,
                   sigma_out=None):
        """harl_dist_rows on this policy's head outputs (Gaussian mean / normalised logits of one or several heads)."""
        net = self.actor
        if net.md and getattr(self, "_head_off", None) is None:
            off = [0]
            for n in net.nvec:
                off.append(off[-1] + int(n))
            self._head_off = torch.tensor(off, dtype=torch.int32, device=self.device)
        log_std, xc, yc, discrete, act_dim = net.dist_args()
        call("harl_dist_rows", ptr(head), M, act_dim, discrete, log_std, xc, yc, ptr(noise), ptr(actions),
             ptr(self._head_off) if net.md else None, len(net.nvec) if net.md else 1, 1, ptr(logp), ptr(probs), ptr(argmax_out),
             ptr(ent_rows), ptr(sigma_out), stream(), tag="dist_rows")

    def evaluate_actions(self, obs, rnn_states_actor, action, masks, available_actions=None, active_masks=None):
        """(action_log_probs [B, act_w], dist_entropy 0-d, action_distribution) as the reference returns them
        (stochastic_policy.py:88-127, act.py:104-157): the entropy is the active-mask-weighted mean over rows when
        ``use_policy_active_masks`` and masks are given, the plain mean otherwise; the distribution is a
        ``torch.distributions`` object built from the head outputs (Gaussian mean / sigma, or normalised masked logits).
        Device tensors, no autograd graph (the update path differentiates inside the kernels)."""
        obs = _as_dev(obs, self.device)
        obs = obs.reshape(obs.shape[0], -1)
        action = _as_dev(action, self.device).reshape(obs.shape[0], -1)
        avail = None if available_actions is None else _as_dev(available_actions, self.device).reshape(obs.shape[0], -1)
        M = obs.shape[0]
        net = self.actor
        out = torch.empty(M, net.act_w, **self.tpdv)
        # zeros, not empty: the distribution object built below validates its parameters, so where the launches are recorded
        # instead of executed (the host-side tests) it must not be handed whatever the allocator's recycled block held
        head = torch.zeros(M, net.act_dim, **self.tpdv)
        net.fold()
        self._logp_pass(obs, action, avail, M, out, head_out=head, rnn_states=rnn_states_actor, masks=masks)
        # entropy rows, their (active-mask-weighted) mean and sigma behind the C ABI (harl_dist_rows / harl_masked_moments /
        # harl_moments_mean); the distribution OBJECT the reference returns is built from the kernel outputs
        ent_rows = torch.empty(M, **self.tpdv)
        sigma = None if net.discrete else torch.ones(net.act_dim, **self.tpdv)  # (a valid scale for the same reason)
        self._dist_rows(head, M, ent_rows=ent_rows, sigma_out=sigma)
        am = None
        if not net.md and active_masks is not None and self.use_policy_active_masks:  # (act.py:117-141: never for MultiDiscrete)
            am = _as_dev(active_masks, self.device).reshape(M).contiguous()
        mom = torch.zeros(3, dtype=torch.float64, device=self.device)
        entropy = torch.empty((), **self.tpdv)
        call("harl_masked_moments", ptr(ent_rows), ptr(am), M, ptr(mom), _lib.scratch("mm"), stream())
        call("harl_moments_mean", ptr(mom), ptr(entropy), stream())
        if net.md:
            return out, entropy, None
        dist = (torch.distributions.Categorical(logits=head) if net.discrete
                else torch.distributions.Normal(head, sigma.expand_as(head)))
        return out, entropy, dist

    @torch.no_grad()
    def get_actions(self, obs, rnn_states_actor, masks, available_actions=None, deterministic=False):
        """Rollout-side sampling (on_policy_base.py:52-69 -> StochasticPolicy.forward, act.py:45-86).  The trunk, GRU
        step and head run on the HIP kernels (head outputs via ``StochasticPolicy.head_logp(head_out=...)``); the draw itself
        uses torch's device generator, which is what the reference's ``Normal.sample()/Categorical.sample()`` use on a
        GPU.  Returns device tensors (actions [B, act_w], action_log_probs [B, act_w], rnn_states [B, 1, H])."""
        net = self.actor
        x = _as_dev(obs, self.device)
        x = x.reshape(x.shape[0], -1)
        M = x.shape[0]
        avail = None if available_actions is None else _as_dev(available_actions, self.device).reshape(M, -1)
        net.fold()
        head = torch.empty(M, net.act_dim, **self.tpdv)
        # (always a device tensor: the reference's callers apply _t2n to it, on_policy_base_runner.py:310-312,533)
        rnn_out = None if rnn_states_actor is None else _as_dev(rnn_states_actor, self.device)
        h = self._logp_pass(x, None, avail, M, None, head_out=head, rnn_states=rnn_states_actor, masks=masks,
                            h_last=True)  # head_out only: no actions needed
        if net.recurrent:
            rnn_out = h.reshape(M, net.recurrent_n, -1).clone()
        # everything around the draw runs in harl_dist_rows; the draw itself is torch's device generator
        if net.discrete:  # head = normalised logits (masked entries ~ -1e10); MultiDiscrete: one draw per head, log-probs summed
            nh = len(net.nvec) if net.md else 1
            actions = torch.empty(M, nh, **self.tpdv)
            logp = torch.empty(M, 1, **self.tpdv)
            if deterministic:
                self._dist_rows(head, M, argmax_out=actions, logp=logp)  # (actions NULL: the log-prob of the argmax)
            else:
                probs = torch.empty_like(head)
                self._dist_rows(head, M, probs=probs)
                if net.md:
                    lo = 0
                    for k, n in enumerate(net.nvec):  # act.py:56-73, one Categorical.sample() per head, in order
                        actions[:, k:k + 1] = torch.multinomial(probs[:, lo:lo + n], 1)
                        lo += n
                else:
                    actions.copy_(torch.multinomial(probs, 1))
                self._dist_rows(head, M, actions=actions, logp=logp)
        else:
            noise = None if deterministic else torch.randn_like(head)
            actions = torch.empty_like(head)
            logp = torch.empty_like(head)
            self._dist_rows(head, M, noise=noise, actions=actions, logp=logp)
        return actions, logp, rnn_out

    @torch.no_grad()
    def act(self, obs, rnn_states_actor, masks, available_actions=None, deterministic=False):
        actions, _, rnn = self.get_actions(obs, rnn_states_actor, masks, available_actions, deterministic)
        return actions, rnn

    def prep_training(self):
        self.actor.train()
        self.actor.invalidate_caches()

    def prep_rollout(self):
        # phase boundary = cache boundary: the folded weights and the normalised-input image are re-derived on first use of
        # every rollout / training phase, so a parameter write that torch's version counter cannot see (``p.data.copy_()``,
        # a raw-pointer kernel, load through DLPack) is picked up at the next prep_rollout() / prep_training() / train()
        self.actor.eval()
        self.actor.invalidate_caches()


class HAPPO(OnPolicyBase):
    def __init__(self, args, obs_space, act_space, device=torch.device("cuda:0")):
        super().__init__(args, obs_space, act_space, device)
        self.clip_param = args["clip_param"]
        self.ppo_epoch = args["ppo_epoch"]
        self.actor_num_mini_batch = args["actor_num_mini_batch"]
        self.entropy_coef = args["entropy_coef"]
        self.use_max_grad_norm = args["use_max_grad_norm"]
        self.max_grad_norm = args["max_grad_norm"]
        self._surrogate_mode = 0  # the loss launches' mode (StochasticPolicy.head_loss): 0 = clipped (HAPPO)
        self._info = torch.zeros(4, dtype=torch.float64, device=self.device)  # fp64 sums of the per-update fp32 policy_loss, dist_entropy, grad_norm, ratio (the reference sums .item() values: happo.py:145-150)
        self._grad_tap = None
        self._trace = None  # test hook: list receiving a clone of the running statistics after every optimiser step
        self._state_tap = None  # test hook: list receiving (parameters, exp_avg, exp_avg_sq, step) as they stand BEFORE every optimiser step
        # runner-internal: the event behind which this agent's sequential-update factor is complete (it is produced on the
        # runner's post-update stream while this agent's first forward already runs, runner.train); awaited in front of the
        # first loss launch -- the only consumer of the factor
        self._factor_ready = None

    def _await_factor(self) -> None:
        ev = self._factor_ready
        if ev is not None:
            self._factor_ready = None
            torch.cuda.current_stream(self.device).wait_event(ev)

    # ---- one optimiser step on rows idx[0..m) of the flat [T*N, .] tensors (happo.py:28-102) ---------
    def _forward_backward(self, obs, idx, m, actions, avail, old_logp, adv, adv_moments, factor, active, seq=None,
                          logp_out=None):
        """Forward, loss and backward of one minibatch: leaves the UNSCALED folded gradients in ``net.dwp`` and the loss
        kernel's per-block partial sums in ``net.part_scalars``.  ``seq`` (recurrent nets): the batch is L x m_pad rows in
        the GRU layout (nets.build_seq), idx = seq['idx'].  ``logp_out`` [m, act_w]: also emit log pi(a|o) under the
        pre-step parameters (by batch position).  ``factor`` None = 1 (MAPPO)."""
        net = self.actor
        s = stream()
        # clip, entropy coefficient, aggregation, surrogate mode: the same four in every loss launch
        loss = (float(self.clip_param), float(self.entropy_coef), int(self.action_aggregation == "mean"), self._surrogate_mode)
        route = net._step_route(idx is None, seq is None, True)
        lead = net.step_forward(route, obs, idx, m, seq)  # the image, or the trunk as far as the route runs it in front of the loss
        self._await_factor()
        if route.kind == "layers":
            mv, mp = (seq["m"], seq["m_pad"]) if seq is not None else (0, 0)
            nblk, head_dw_done = net.head_loss(m, idx, actions, avail, old_logp, adv, adv_moments, factor, active, *loss, mv, mp,
                                               logp_out, md_ent_scale=lambda: self._md_ent_scale(idx, m, active, seq))
        else:  # the loss launches of csrc/update.hip ("last": over the rows idx gathers); both leave the head's weight gradient
            fused = route.kind == "fused"
            call("harl_update_fwd_actor" if fused else "harl_update_last_actor", *lead, *net.dist_args(),
                 *(() if fused else (ptr(idx),)), ptr(actions), ptr(avail), ptr(old_logp), ptr(adv), ptr(adv_moments), ptr(factor),
                 ptr(active), *loss, ptr(logp_out), *net.step_outputs(route), s, tag="update_fwd" if fused else "update_last")
            nblk, head_dw_done = net.n_wg, True
        net.step_backward(route, obs, idx, m, seq, head_dw_done)
        return nblk  # rows of part_scalars

    def _md_ent_scale(self, idx, m, active, seq) -> Optional[torch.Tensor]:
        """MultiDiscrete: device scalar sum(active) / rows of the (global) minibatch.  The reference's entropy bonus there is
        (1/rows) sum_rows sum_heads H while the surrogate is divided by sum(active) (act.py:126-139, happo.py:77-81); the
        optimiser kernel applies ONE scale 1 / sum(active) to the whole gradient, so the entropy part carries this ratio.
        None (= 1) without active masks."""
        if active is None:
            return None
        if getattr(self, "_md_ent_override", None) is not None:  # parameter sharing: the ratio of the concatenated batch
            return self._md_ent_override
        if seq is not None:      # L x m_pad rows, padding rows addressed through idx but not counted
            j = torch.arange(m, device=self.device)
            live = (j % seq["m_pad"]) < seq["m"]
            rows = idx[live] if idx is not None else j[live]
            st = torch.stack([active[rows].sum(), torch.tensor(float(rows.numel()), device=self.device)])
        else:
            a = active if idx is None else active[idx]
            st = torch.stack([a.sum(), torch.tensor(float(m), device=self.device)])
        self.comm.all_reduce_sum(st)
        return (st[0] / st[1]).reshape(1).contiguous()

    def _optimizer_step(self, nblk: Optional[int]):
        """[data-parallel all-reduce] + fused scalar reduce / unfold / grad-norm / clip / Adam / re-fold.  ``nblk`` None:
        ``net.scalars`` already holds the summed loss scalars (several minibatch segments were accumulated)."""
        net = self.actor
        net._ensure_ws(1)
        sc = net.scalars
        if self._state_tap is not None:  # (the full-size checks re-run every update of the oracle from exactly this state)
            o = self.actor_optimizer
            self._state_tap.append((net.flat_param.clone(), o.exp_avg.clone(), o.exp_avg_sq.clone(), o.step_count))
        if nblk == 0:  # this rank holds no row of the (global) minibatch: contribute zeros to the all-reduce
            net.dwp.zero_()
            sc.zero_()
            nblk = None
        ps_kw = dict(part_scalars=net.part_scalars, n_scalar_blocks=nblk) if nblk is not None else {}
        if net.gauss_wide:  # (nblk None: the segments' sums were accumulated, as net.scalars)
            self._refuse_gauss_wide_dp()
            if nblk is not None:
                net.ls_reduce(nblk, accumulate=False)
            ps_kw["ls_sum"] = net.ls_sum
        if self.comm.enabled:  # ONE collective per optimiser step: [folded gradients | loss scalars] (dist.py)
            hilo = net.dwp_msg[net.total_dwp:]
            if nblk is not None:  # partial rows -> fp64 sums -> fixed-grid fp32 pieces behind the gradients, one launch
                call("harl_reduce_pack_scalars", ptr(net.part_scalars), nblk, ptr(sc), ptr(hilo), stream())
            else:
                call("harl_pack_scalars_hilo", ptr(sc), ptr(hilo), stream())
            self.comm.all_reduce_message(net.dwp_msg)
            ps_kw = dict(scalars_hilo=hilo)
        # loss = sum / sum(active) (happo.py:77-85): gradients are linear in 1/sum(active), applied inside the kernel
        ls_off = -1 if net.discrete else net.offsets["act.action_out.log_std"][0]
        self.actor_optimizer.step(0, 0.0, self.use_max_grad_norm, self.max_grad_norm, self._info, ls_off, net.act_dim,
                                  **ps_kw)
        if self._trace is not None:  # test hook: per-update statistics = differences of these snapshots (no host sync)
            self._trace.append(self._info.clone())
        if self._grad_tap is not None:  # test hook: scaled, pre-clip gradient of this update (host sync)
            self._grad_tap(net.flat_grad * float(1.0 / sc[1].item()), sc.clone())

    def _update_core(self, obs, idx, m, actions, avail, old_logp, adv, adv_moments, factor, active, seq=None,
                     logp_out=None, _graph=False):
        def step():
            nblk = self._forward_backward(obs, idx, m, actions, avail, old_logp, adv, adv_moments, factor, active, seq=seq,
                                          logp_out=logp_out)
            self._optimizer_step(nblk)
        if not _graph:
            if (self.actor.cat_wide or self.actor.gauss_wide) and graphs.enabled():  # HARL_GRAPH=1: these heads run eagerly, and say so
                self._graph.eager_steps += 1
            return step()
        # HARL_GRAPH=1 (graphs.py): replay this step from a hipGraph.  Eager all the same: the epoch-0 step that also emits the
        # pre-update log-probs, steps under a test hook (they read back / clone between the launches), instrumented steps.
        G, net, opt = self._graph, self.actor, self.actor_optimizer
        if (seq is not None or self._trace is not None or self._grad_tap is not None
                or self._state_tap is not None or not graphs.launches_capturable(self.device) or opt.hyper_rows_left() < 1):
            return G.eager(step)
        warm = (m, idx is None, avail is None, adv_moments is None, factor is None, active is None) + self._graph_consts()
        if logp_out is not None:
            # never captured (the output exists in the first epoch only) -- but it is the launch sequence of the later epochs,
            # kernel for kernel and size for size (log-probs are one more pointer to the same loss launch), so it has raised
            # every LDS limit they need: it counts as their eager first run
            G.eager(step)
            G.warm.add(warm)
            return
        self._await_factor()          # (cross-stream waits stay in front of the region)
        net.prepare_x0n(obs, idx, m)  # ... and so does the launch that depends on a host-side cache
        if self._graph_gen != net._ws_gen:
            G.drop()
            self._graph_gen = net._ws_gen
        p = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        key = warm + (p(obs), p(idx), p(actions), p(avail), p(old_logp), p(adv), p(adv_moments), p(factor), p(active),
                      p(self._info), p(net.flat_param), p(net.pack_arena), p(opt.exp_avg), p(opt._hyper_dev), opt._hyper_rows)
        G.run(warm, key, step, opt)

    def _graph_consts(self) -> tuple:
        """Host scalars and routing switches that are baked into the launches of an optimiser step."""
        g = self.actor_optimizer.param_groups[0]
        return (float(self.clip_param), float(self.entropy_coef), self.action_aggregation, self._surrogate_mode,
                bool(self.use_max_grad_norm), float(self.max_grad_norm), tuple(g["betas"]), float(g["eps"]),
                float(g["weight_decay"])) + routing_switches()

    def update(self, sample):
        """API-compatible single update on an already-gathered minibatch (tuple order of happo.py:37-48).
        Returns (policy_loss, dist_entropy, actor_grad_norm, mean importance weight) as 0-d device tensors."""
        (obs, _rnn, actions, _masks, active, old_logp, adv, avail, factor) = sample
        dev = self.device
        obs = _as_dev(obs, dev)
        m = obs.shape[0]
        before = self._info.clone()
        self.actor.fold()
        seq, idx, rows = None, None, m
        if self.actor.recurrent:  # gathered [L*m, .] l-major minibatch + rnn_states [m, 1, H] (recurrent generators)
            HS = self.actor.hidden_sizes[-1] * self.actor.recurrent_n
            nseq = _as_dev(_rnn, dev).shape[0]
            seq = build_seq(dev, m // nseq, nseq, HS, h0=_as_dev(_rnn, dev).reshape(nseq, HS), masks_src=_as_dev(_masks, dev))
            idx, rows = seq["idx"], seq["L"] * seq["m_pad"]
        self._update_core(obs.reshape(m, -1), idx, rows, _as_dev(actions, dev).reshape(m, -1),
                          None if avail is None else _as_dev(avail, dev).reshape(m, -1),
                          _as_dev(old_logp, dev).reshape(m, -1), _as_dev(adv, dev).reshape(m), None,
                          None if factor is None else _as_dev(factor, dev).reshape(m),
                          _as_dev(active, dev).reshape(m) if self.use_policy_active_masks else None, seq=seq)
        d = self._info - before
        return d[0], d[1], d[2], d[3]

    _INFO_KEYS = ("policy_loss", "dist_entropy", "actor_grad_norm", "ratio")

    def masked_moments(self, actor_buffer: OnPolicyActorBuffer, advantages, out: torch.Tensor) -> None:
        """fp64 {sum, sumsq, count} of ``advantages`` over this agent's active entries (happo.py:119-127) -> out[3]."""
        T, N = actor_buffer.actions.shape[:2]
        adv = _as_dev(advantages, self.device).reshape(T * N)
        call("harl_masked_moments", ptr(adv), ptr(actor_buffer.flat("active_masks")), T * N, ptr(out), _lib.scratch("mm"), stream())

    def rng_footprint(self, actor_buffer: OnPolicyActorBuffer) -> list:
        """Sizes of the ``torch.randperm`` draws ONE train() of this actor takes from the global CPU generator, in order (one
        per epoch: on_policy_actor_buffer.py:131 / :196 / :241 over the GLOBAL buffer).  The runner fast-forwards the
        generator over them to start the critic's update -- whose samplers draw AFTER every actor's in the reference --
        next to the actors' (runner.train, round 6)."""
        T, N = actor_buffer.actions.shape[:2]
        n_g = self.shard[0] if self.shard else N
        if self.use_recurrent_policy:
            size = (T * n_g) // self.data_chunk_length
        elif self.use_naive_recurrent_policy:
            size = n_g
        else:
            size = T * n_g
        return [size] * self.ppo_epoch

    def fuses_old_logp(self) -> bool:
        """True when train()'s first forward sees every buffer row, in order, under the pre-update parameters -- i.e. it
        computes exactly what the runner's pre-update log-prob pass computes (on_policy_ha_runner.py:66-83)."""
        return self.actor_num_mini_batch == 1 and not (self.use_recurrent_policy or self.use_naive_recurrent_policy)

    def train(self, actor_buffer: OnPolicyActorBuffer, advantages, state_type, _pre=None, _defer=False,
              _old_logp_out=None):
        """ppo_epoch x actor_num_mini_batch updates (happo.py:104-158).  ``advantages`` is the raw [T, N, 1]
        advantage tensor; the per-agent masked normalisation (happo.py:122-127) is folded into the loss kernel
        through the fp64 moments {sum, sumsq, count}.
        Runner-internal: ``_pre = (moments[3] device fp64, count)`` when the runner already reduced the moments of all
        agents with one read-back; ``_defer`` returns the averaged statistics as a device tensor (resolved by the
        runner in one transfer at the end of train()) and leaves deferred RNG advances pending; ``_old_logp_out``
        [T*N, act_w] receives the pre-update log-probs from the first epoch's forward (only if ``fuses_old_logp()``)."""
        dev = self.device
        buf = actor_buffer
        T, N = buf.actions.shape[:2]
        B = T * N
        if _pre is None:  # called directly (the runner invalidates once, before its own pre-update log-prob pass)
            self.actor.invalidate_caches()
        train_info = {k: 0.0 for k in self._INFO_KEYS}
        adv = _as_dev(advantages, dev).reshape(B).contiguous()
        active = buf.flat("active_masks").reshape(B)
        if _pre is None:
            moments = torch.zeros(3, dtype=torch.float64, device=dev)
            self.masked_moments(buf, adv, moments)
            self.comm.all_reduce_sum(moments)
            count = float(moments[2].item())
        else:
            moments, count = _pre
        if count == 0.0:  # np.all(active_masks[:-1] == 0) early-out (happo.py:119-120)
            return train_info
        if state_type != "EP":  # FP: the runner already normalised over all agents (on_policy_ha_runner.py:36-45)
            moments = None
        self._info.zero_()
        buf.__dict__.pop("_seq_cache", None)  # the recurrent samplers' per-update table never outlives one train() (buffers._recurrent_seqs)
        self.actor.fold()
        obs = buf.flat("obs")
        actions = buf.flat("actions")
        avail = None if buf.available_actions is None else buf.flat("available_actions")
        old_logp = buf.flat("action_log_probs")
        factor = None if buf.factor is None else buf.factor.reshape(B)  # None: MAPPO (no sequential-update factor)
        n_global = self.shard[0] * T if self.shard else B
        graph = False
        if self._graph_config_ok():
            # HARL_GRAPH=1: the Adam scalars of the coming steps go to the device once (FusedAdam.begin_steps); what arrives as a
            # fresh tensor per call -- advantages, their moments, the factor -- moves into persistent buffers, because a
            # captured step holds addresses
            self.actor_optimizer.begin_steps(self.ppo_epoch * self.actor_num_mini_batch)
            graph = graphs.launches_capturable(dev)
        if graph:
            self._await_factor()
            adv, moments, factor = (self._graph_stage("adv", adv), self._graph_stage("moments", moments),
                                    self._graph_stage("factor", factor))
        try:
            self._train_epochs(buf, obs, actions, avail, old_logp, adv, moments, factor, active, B, n_global, _old_logp_out, graph)
        finally:
            self.actor_optimizer.end_steps()
        n_upd = self.ppo_epoch * self.actor_num_mini_batch
        if _defer:
            return self._info / n_upd
        rng_sync()
        vals = (self._info / n_upd).cpu().tolist()  # the single read-back of this agent's update
        for k, v in zip(self._INFO_KEYS, vals):
            train_info[k] = v
        return train_info

    def _train_epochs(self, buf, obs, actions, avail, old_logp, adv, moments, factor, active, B, n_global, _old_logp_out,
                      graph: bool) -> None:
        dev = self.device
        for epoch in range(self.ppo_epoch):
            if self.use_recurrent_policy or self.use_naive_recurrent_policy:
                for seq in buf.recurrent_batches(self.actor_num_mini_batch, self.data_chunk_length,
                                                 naive=not self.use_recurrent_policy, shard=self.shard):
                    if seq.get("empty"):
                        self._optimizer_step(0)
                        continue
                    self._update_core(obs, seq["idx"], seq["L"] * seq["m_pad"], actions, avail, old_logp, adv, moments,
                                      factor, active if self.use_policy_active_masks else None, seq=seq)
                continue
            if self.actor_num_mini_batch == 1:
                # the single "minibatch" is the whole (local) buffer: the sums do not depend on the order, so only the
                # generator state is replayed (bit-exact RNG stream), not the 819200-element shuffle itself
                consume_randperm(n_global)
                self._update_core(obs, None, B, actions, avail, old_logp, adv, moments, factor,
                                  active if self.use_policy_active_masks else None,
                                  logp_out=_old_logp_out if epoch == 0 else None, _graph=graph)
                continue
            sampler = minibatch_indices(n_global, self.actor_num_mini_batch, dev)  # CPU RNG draw, bit-exact with the reference
            for ind in sampler:
                if self.shard:
                    ind = local_minibatch_rows(ind, self.shard[0], self.shard[1], self.shard[2])
                    if ind.numel() == 0:
                        self._optimizer_step(0)
                        continue
                # (graph mode: every minibatch's rows go through ONE persistent index buffer, minibatches are of equal size)
                self._update_core(obs, self._graph_stage("idx", ind) if graph else ind.to(dev), ind.numel(), actions, avail,
                                  old_logp, adv, moments, factor, active if self.use_policy_active_masks else None, _graph=graph)


class HAA2C(HAPPO):
    """HAPPO without ratio clipping, ``a2c_epoch`` epochs (reference: harl/algorithms/actors/haa2c.py:10-153)."""

    def __init__(self, args, obs_space, act_space, device=torch.device("cuda:0")):
        a = dict(args)
        a.setdefault("clip_param", 0.0)   # unused by the unclipped surrogate
        a.setdefault("ppo_epoch", a["a2c_epoch"])
        super().__init__(a, obs_space, act_space, device)
        self.args = args
        self.a2c_epoch = self.ppo_epoch = args["a2c_epoch"]
        self._surrogate_mode = 2
