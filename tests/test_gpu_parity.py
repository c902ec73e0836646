"""-m gpu: parity of the HIP path (through the C ABI) against the oracle and the reference's golden vectors."""
import os

import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5  # BASELINE.json: fp32 losses / grad-norms within 1e-5 relative for identical buffer contents
# Whole-train() comparisons against the reference's golden vectors use the SAME 1e-5 bar, entry by entry (every optimiser
# step's loss / entropy / grad-norm / ratio, the averaged infos, the final parameters), except where the reference's own
# fp32 figure is further than that from exact arithmetic: oracle/gen_noise_floor.py re-runs each golden case in float64
# (tests/golden/noise/*.npz), and an entry may differ from the reference by at most
#     max(1e-5, 2 x max(|reference_fp32 - fp64| / |fp64|, how far the reference's figure moves when its own gradient rounding
#                       errors get another sign pattern and its parameters one ulp of noise per step))
# -- e.g. the first policy loss of `a2c_box_h64` is a near-zero masked mean of advantage-normalised surrogates and the
# reference itself is 1.0e-4 away from its exact value.  check_train_golden reports that ratio as `*_excess` (<= 1 passes).


def _G():
    from tests import gpu_checks
    return gpu_checks


# Absolute ceilings on RAW figures that are otherwise reported only ('_' prefix) next to their *_excess ratio: the
# excess bar scales with the oracle's own measured noise, so on an ill-conditioned case a gross error in the CG / FVP / tangent
# kernels could hide behind a large noise floor.  These do not replace the excess bars; they cap what "noise" may mean.
RAW_CEILINGS = (("cg_step_dir_vec_rel", 1e-3), ("fvp_vec_rel", 1e-4), ("surrogate_grad_vec_rel", 1e-4),
                ("actor_grad_vec_rel", 1e-4), ("critic_grad_vec_rel", 1e-4), ("logp_vec_rel", 1e-4), ("values_vec_rel", 1e-4))


def _assert_all(res, tol=TOL, exact_keys=("mismatch", "perm_", "count")):
    for k, v in res.items():
        if k.startswith("_") and isinstance(v, float) and not k.startswith("_unmasked"):
            for name, cap in RAW_CEILINGS:
                if k[1:] == name or k[1:].endswith("_" + name):
                    assert v < cap, (k, v, "raw ceiling", cap)
        if k.startswith("_") or not isinstance(v, float):
            continue
        if any(e in k for e in exact_keys):
            assert v == 0.0, (k, v)
        elif k.endswith("_excess"):
            assert v <= 1.0, (k, v)   # within max(1e-5, 2 x the reference's own measured uncertainty) on every entry
        else:
            assert v < tol, (k, v)


def test_gae_bit_exact_all_branches():
    res = _G().check_gae()
    assert all(v == 0.0 for v in res.values()), {k: v for k, v in res.items() if v}


def test_elementwise_kernels():
    _assert_all(_G().check_elementwise(), tol=2e-6)


def test_wide_input_first_layer():
    """x0n image / LayerNorm statistics / split-bf16 GEMM of the wide-observation path at widths 65..512."""
    _assert_all(_G().check_wide_input(), tol=5e-6)


def test_wide_gemm_with_shared_weight_panels_is_bit_identical():
    """k_fwd_wide_sh (weight fragments through LDS, round 5) vs the streaming k_fwd_wide on the same inputs: bit for bit."""
    for k, v in _G().check_wide_shared().items():
        assert v == 0.0, (k, v)


def test_fused_gradnorm_clip_adam():
    _assert_all(_G().check_adam(), tol=2e-6)


@pytest.mark.parametrize("i", range(14))
def test_mlp_forward_logp_and_values(i):
    G = _G()
    _assert_all(G.check_forward(G.FWD_SHAPES[i]), tol=TOL)


@pytest.mark.parametrize("i", range(14))
def test_single_update_gradients(i):
    G = _G()
    _assert_all(G.check_gradients(G.FWD_SHAPES[i]), tol=TOL)


def test_single_update_gradients_mean_aggregation_inactive_agents():
    G = _G()
    _assert_all(G.check_gradients(G.FWD_SHAPES[0], agg="mean", inactive_p=0.3), tol=TOL)


@pytest.mark.parametrize("name", ["mpe_box_h64", "mpe_box_h128", "mpe_disc_h64", "cheetah_h128x3_mb2",
                                  "box_mean_inactive_novn", "wide_obs_h64", "a2c_box_h64", "fp_box_h64",
                                  "fp_disc_h128_mb2", "disc50_h128", "hands_h256x3", "hands_h256x3_mb2_fp"])
def test_train_matches_reference_golden(name):
    _assert_all(_G().check_train_golden(name), tol=TOL)


@pytest.mark.parametrize("i", [0, 1, 2, 4])
def test_hatrpo_gradient_fvp_and_update(i):
    """HATRPO: surrogate gradient, Fisher-vector product (tangent pass + backward) and one full update (CG + line search)
    vs the oracle's autograd double backward.  CG amplifies rounding differences: the step direction is held to the symmetric
    bar of check_trpo_upstream (``cg_step_dir_excess``: distance from the float64 solve <= 4 x the fp32 oracle's own)."""
    G = _G()
    _assert_all(G.check_trpo(G.FWD_SHAPES[i]), tol=TOL)


@pytest.mark.parametrize("act", ["tanh", "selu", "leaky_relu", "sigmoid"])
def test_hatrpo_activation_gradient_fvp_and_update(act):
    """HATRPO on networks built with an activation other than relu (round 4): the Fisher-vector product's tangent pass composed
    from raw GEMMs + harl_act_ln_tangent, against the oracle's autograd double backward; one full update (CG + line search)."""
    G = _G()
    spec = dict(G.FWD_SHAPES[0])
    spec["over"] = dict(spec.get("over", {}), activation_func=act)
    _assert_all(G.check_trpo(spec), tol=TOL)


@pytest.mark.parametrize("i", [0, 1, 2])
def test_hatrpo_gru_gradient_fvp_and_update(i):
    """HATRPO with GRU policies: the Fisher-vector product through the recurrence (forward-mode tangent kernel + BPTT)
    against the oracle's double backward, padded (m = 40), identity (m = 64) and ragged (m = 7, mixed widths) layouts."""
    G = _G()
    # everything update() reports after the CG solve (*_excess) is held to max(1e-5, 2 x the oracle's own measured
    # uncertainty), the CG direction to 4 x the oracle's own distance from the float64 solve -- gpu_checks._trpo_update_excess;
    # gradient, FVP and surrogate loss: check_trpo_rnn's own *_excess (distance from float64 against the fp32 oracle's)
    _assert_all(G.check_trpo_rnn(G.RNN_SHAPES[i]), tol=TOL)


@pytest.mark.parametrize("i", [7, 8])
def test_hatrpo_width256_gradient_fvp_and_update(i):
    """HATRPO on 256-wide layers (round 4): the tangent pass on the K-panel kernel (harl_mlp_panel_tangent) and the 256-wide
    instantiation of the head FVP kernel, against the oracle: three layers / Box(20) / 211 inputs, two layers / Discrete(6)."""
    G = _G()
    _assert_all(G.check_trpo(G.FWD_SHAPES[i]), tol=TOL)


@pytest.mark.parametrize("i", [0, 1])
def test_hatrpo_composed_gru_gradient_fvp_and_update(i):
    """HATRPO on a 128-wide GRU and on two stacked 64-wide GRU layers (round 4): the Fisher-vector product's tangent through the
    per-step composition (gru_wide.tangent: raw GEMMs + harl_gru_cell_tangent) against the oracle's double backward."""
    G = _G()
    _assert_all(G.check_trpo_rnn(G.TRPO_RNN_WIDE_SHAPES[i]), tol=TOL)


@pytest.mark.parametrize("name", ["trpo_box_h64", "trpo_disc_h64", "trpo_wide_h128x3", "trpo_rnn_disc_h64", "trpo_rnn_box_h64",
                                  "trpo_rnn_fp_disc36_h64", "trpo_box_h128_tanh", "trpo_disc_h64_selu", "trpo_rnn_box_h128",
                                  "trpo_rnn2_disc_h64", "trpo_box_h256x2"])
def test_hatrpo_train_matches_reference_golden(name):
    _assert_all(_G().check_train_golden(name), tol=TOL)


@pytest.mark.parametrize("i", [0, 1, 5, 7])
def test_rollout_get_actions(i):
    G = _G()
    res = G.check_get_actions(G.FWD_SHAPES[i])
    for k, v in res.items():
        if "count" in k or "mismatch" in k:
            assert v == 0.0, (k, v)
        elif "zscore" in k:
            assert v < 0.05, (k, v)
        else:
            assert v < TOL, (k, v)


@pytest.mark.parametrize("i", range(4))
def test_gru_policy_forward_and_update(i):
    """GRU policies (rnn.py): L-step unroll with mask resets, BPTT, shared-LayerNorm unfold -- one actor and one critic
    update vs the oracle; padded (m % 32 != 0) and identity sequence layouts, single-step rollout calls.  Every figure is held
    to max(1e-5, 2 x the fp32 oracle's own distance from the same update in float64) (``*_excess``)."""
    G = _G()
    _assert_all(G.check_rnn_update(G.RNN_SHAPES[i]), tol=TOL)


@pytest.mark.parametrize("name", ["rnn_box_h64", "rnn_disc_h64_mb2", "rnn_naive_h64", "rnn_fp_box_h64_mb2",
                                  "rnn_naive_fp_disc_h64", "rnn_fp_disc36_h64"])
def test_recurrent_train_matches_reference_golden(name):
    """Chunked and naive recurrent samplers + GRU actor/critic through a whole OnPolicyHARunner.train() vs the reference."""
    _assert_all(_G().check_train_golden(name), tol=TOL)


@pytest.mark.parametrize("name", ["rnn_box_h64", "rnn_disc_h64_mb2", "rnn_naive_fp_disc_h64"])
def test_composed_gru_matches_64_wide_goldens(name, monkeypatch):
    """The per-step composition (layer GEMMs + element-wise cell kernels) on 64-wide GRUs against the goldens the fused kernels
    are held to: checks harl_amd/gru_wide.py independently of anything 128-wide."""
    monkeypatch.setenv("HARL_GRU_COMPOSED", "1")
    _assert_all(_G().check_train_golden(name), tol=TOL)


@pytest.mark.parametrize("name", ["rnn_box_h128", "rnn_disc_h128_mb2", "rnn2_box_h64", "rnn2_disc_h128_naive_mb2"])
def test_gru128_train_matches_reference_golden(name, monkeypatch):
    """GRU policies on 128-wide layers (the default hidden_sizes with use_recurrent_policy) and stacked GRU layers
    (recurrent_n = 2, rnn.py:14; 64-wide chunked, 128-wide naive with two mini-batches) vs the reference."""
    _assert_all(_G().check_train_golden(name), tol=TOL)


@pytest.mark.parametrize("name", ["mpe_box_h128_tanh", "disc_h64_selu_mb2", "wide_fp_box_h128_64_leaky", "a2c_box_h64x3_sigmoid",
                                  "mappo_shared_disc_h128_tanh"])
def test_activation_train_matches_reference_golden(name):
    """activation_func other than relu (models_tools.py:28-50): whole train() against fixtures recorded from the reference --
    tanh, selu with mini-batches and unavailable actions, leaky_relu on 77-wide inputs with the FP critic and mixed widths,
    sigmoid under HAA2C on three layers, tanh under MAPPO with shared parameters."""
    _assert_all(_G().check_train_golden(name), tol=TOL)


@pytest.mark.parametrize("act", ["tanh", "sigmoid", "leaky_relu", "selu"])
@pytest.mark.parametrize("i", [0, 4])
def test_activation_forward_and_single_update(act, i):
    """Every supported activation on the MPE shape and on the 393-wide three-layer shape: log-probs / values, then ONE
    HAPPO.update + VCritic.update (gradient vectors, loss scalars, post-Adam parameters) vs the oracle."""
    G = _G()
    spec = dict(G.FWD_SHAPES[i], over=dict(activation_func=act))
    _assert_all(G.check_forward(spec), tol=TOL)
    _assert_all(G.check_gradients(spec), tol=TOL)


@pytest.mark.parametrize("discrete,recurrent", [(False, False), (True, False), (False, True)])
def test_rollout_loop_learns_on_toy_env(discrete, recurrent):
    """run(): device-side collect/insert around a host environment, then the update; rewards must improve."""
    res = _G().check_rollout_learning(discrete, recurrent)
    assert res["nonfinite_count"] == 0.0
    assert res["_improvement"] > (0.08 if discrete else 0.03), res
    assert abs(res["mask_zero_frac"] - 0.04) < 1e-6, res           # every 25th step
    assert abs(res["bad_zero_frac"] - 0.04) < 1e-6, res
    assert abs(res["active_zero_frac_agent1"] - 0.12) < 1e-6, res  # agent 1 is dead 3 steps out of 25


@pytest.mark.parametrize("name", ["md_h64_mb2", "md_lag_h128", "md_rnn_h64", "md_mappo_mean_h64", "md_a2c_h128_64"])
def test_multidiscrete_train_matches_reference_golden(name):
    """MultiDiscrete action spaces (act.py:35-43,117-141; csrc/multihead.hip): whole train() vs the reference -- mini-batches,
    the LAG layout [41, 41, 41, 30] (two logits images), a GRU policy, MAPPO (shared parameters, `mean` aggregation), HAA2C."""
    _assert_all(_G().check_train_golden(name), tol=TOL)


@pytest.mark.parametrize("nvec,hidden", [([5, 3, 4], [64, 64]), ([41, 41, 41, 30], [128, 128])])
def test_multidiscrete_rollout_and_evaluate(nvec, hidden):
    """get_actions / evaluate_actions for MultiDiscrete heads vs the oracle: per-head normalised logits, summed log-probs,
    the reference's entropy figure, deterministic mode = per-head argmax, sampled actions inside their ranges."""
    res = _G().check_multidiscrete_rollout(nvec, hidden)
    for k, v in res.items():
        if "mismatch" in k:
            assert v == 0.0, (k, v)
        else:
            assert v < TOL, (k, v)


@pytest.mark.parametrize("name", ["mappo_box_h64", "mappo_shared_disc_h64_mb2", "mappo_shared_fp_box_h128",
                                  "mappo_shared_rnn_disc_h64_mb2", "mappo_shared_rnn_naive_fp_box_h128"])
def test_mappo_train_matches_reference_golden(name):
    """MAPPO through the same kernels (factor = NULL); parameter sharing accumulates every agent's segment before one
    optimiser step; OnPolicyMARunner.train() vs the reference (incl. its stray randperm(num_agents) draw)."""
    _assert_all(_G().check_train_golden(name), tol=TOL)


def test_checkpoint_compat_with_reference_files(tmp_path):
    """restore() loads checkpoints written by the reference's save(); save() writes what the reference's restore() reads."""
    res = _G().check_checkpoint_compat(str(tmp_path))
    for k, v in res.items():
        if "mismatch" in k:
            assert v == 0.0, (k, v)
        elif "max_abs" in k:
            assert v == 0.0, (k, v)   # parameters are copied, not recomputed
        else:
            assert v < TOL, (k, v)


# every per-update figure of a teacher-forced full-size check that is NOT a cancelling sum: held to 1e-5 FLAT (BASELINE.json's
# letter), on all 15 / 30 / 40 optimiser steps -- next to the measured bars of _assert_all
FORCED_FLAT = ("_actor_update_policy_loss_rel", "_actor_update_dist_entropy_rel", "_actor_update_grad_norm_rel", "_actor_update_ratio_rel",
               "_actor_infos_rel", "_actor_final_param_vec_rel_max", "_critic_final_param_vec_rel")


def _assert_forced_flat(res, keys=FORCED_FLAT, tol=TOL):
    assert res["_teacher_forced"] == 1.0
    for k in keys:
        assert res[k] < tol, (k, res[k])


def test_bench_configuration_against_oracle():
    """One whole bench step (compute + train, 5 + 5 epochs, the bench's own recipe buffers) at T = 200, N = 4096 against the fp32
    oracle on identical buffer contents (gpu_checks.check_bench_config_parity).  Round 6: TEACHER-FORCED -- the oracle re-runs
    every one of the 15 + 5 optimiser steps from the HIP path's own state in front of that step (parameters + Adam moments), so
    every update is a comparison from identical inputs: policy loss, entropy, grad-norm, ratio of all 15 actor updates, the critic's
    5, the averaged statistics and the final parameters within 1e-5 FLAT (measured: <= 3.2e-6), returns / generator state
    bit-exact.  (The free-running form of this check -- one oracle trajectory next to one HIP trajectory -- is chaotic on these
    buffers: profiles/r06_free_running_spread.md.)"""
    res = _G().check_bench_config_parity()
    print("bench-config parity:", {k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in res.items()})
    _assert_all(res)
    _assert_forced_flat(res)


def test_bench_configuration_onpolicy_against_oracle():
    """The same whole step with ON-POLICY stored log-probs (`bench.py --logp onpolicy`: log pi(a|o) + 0.05 N(0,1) under the
    initial weights, importance ratios ~ 1 -- the regime PPO actually runs in).  Measured on MI355X
    (profiles/r05_parity_bench_config_onpolicy.json): this variant is WORSE conditioned than the recipe one, not better --
    the policy loss is a masked mean of advantage-normalised surrogates with ratios ~ 1, i.e. ~ 0 by construction, and the
    gradient a sum of 819 200 terms that cancel to ~1e-3 of their mass: the fp32 oracle's own grad-norms sit 2.2e-3 from its
    float64 twin over the 15 updates (HIP: 4.1e-3 from the fp32 oracle, 0.92 of the bar), its policy losses 1.2e-2 (HIP 7.6e-3).
    What does not divide by a near-zero number is held to 1e-5 FLAT: every update's entropy, the critic throughout, the first
    update's entropy / grad-norm / ratio; the first update's policy loss (|value| ~ 2e-3) to 1e-7 absolute; the rest keeps the
    measured bar."""
    res = _G().check_bench_config_parity(logp="onpolicy")
    print("bench-config parity (on-policy):", {k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in res.items()})
    _assert_all(res)
    # teacher-forced (round 6): what is not a cancelling sum is flat 1e-5 on EVERY update; policy losses and grad-norms ride the
    # measured bar even from identical inputs (the fp32 oracle's own float64 twin: 2.4e-5 / 2.1e-5; HIP 2.0e-5 / 1.2e-5)
    _assert_forced_flat(res, ("_actor_update_dist_entropy_rel", "_actor_update_ratio_rel", "_actor_infos_rel",
                              "_actor_final_param_vec_rel_max", "_critic_final_param_vec_rel"))
    assert res["_actor_update_policy_loss_rel"] < 1e-4 and res["_actor_update_grad_norm_rel"] < 1e-4, res
    for k in ("_actor_update_dist_entropy_rel", "_first_update_dist_entropy_rel", "_first_update_grad_norm_rel", "_first_update_ratio_rel"):
        assert res[k] < TOL, (k, res[k])
    # the first update's policy loss is ~2e-3 (a mean of unit-scale terms that cancel): 1e-7 ABSOLUTE = 1e-7 of the terms' scale
    assert res["_first_update_policy_loss_abs"] < 1e-7, res["_first_update_policy_loss_abs"]


def test_cheetah6_full_size_against_oracle():
    """BASELINE configs[2] at one GPU's share and at FULL size -- HalfCheetah-6x1, 6 agents, T = 200, 4096 rollout threads
    (819 200 rows per agent), MLP [128, 128, 128], 5 + 5 epochs -- against the fp32 oracle on identical buffer contents
    (VERDICT r04 item 3c): the oracle's entry to `harl_update_last_*` (the last hidden layer inside the loss launch, cheetah6's
    hot kernel) and to the layer-by-layer backward of a three-layer trunk at 25 slabs per wave.  Same bars as the MPE bench
    configuration: returns / generator state bit-exact, first update and critic 1e-5 flat, the rest pooled measured bars (the
    oracle in float64 and one one-ulp twin run next to the fp32 run, in worker processes on the box's host cores)."""
    res = _G().check_bench_config_parity(workload="cheetah6")
    print("cheetah6 full-size parity:", {k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in res.items()})
    _assert_all(res)
    _assert_forced_flat(res)  # teacher-forced (round 6): all 30 + 5 updates within 1e-5 flat (measured: <= 1.5e-6)


def test_smac3s5z_full_size_against_oracle():
    """BASELINE configs[3] at FULL size -- SMAC 3s5z shape, 8 agents, T = 160, 512 rollout threads, MLP [64, 64, 64] + GRU,
    Discrete(14) with 30 % unavailable actions, chunks of 10, 5 + 5 epochs -- against the fp32 oracle on identical buffer
    contents: the oracle's entry to the four-waves-per-slab GRU kernels at their measured size (256 training chains per launch,
    full-length log-prob passes of 160 dependent steps), to `harl_build_seq` and to the recurrent critic.  Returns / generator
    state bit-exact; the critic and the first update on the recurrent fixtures' 2e-5 / measured bars (nothing downstream of a
    160-step recurrence is held to 1e-5 flat); the rest on the pooled measured bars."""
    res = _G().check_bench_config_parity(workload="smac3s5z", n_threads=512)
    print("smac3s5z full-size parity:", {k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in res.items()})
    _assert_all(res, tol=2e-5)
    # teacher-forced (round 6): every actor figure of all 40 updates and the recurrent critic's 5 within 1e-5 FLAT
    # (measured: <= 1.8e-6; free-running in round 5: the critic's grad-norms 2.8e-5 where the oracle's own twin sat 4e-5 away)
    _assert_forced_flat(res, FORCED_FLAT + ("_critic_update_grad_norm_rel", "_critic_update_value_loss_rel"))


def _assert_trpo_full_size(res, tol=TOL):
    _assert_all(res, tol=tol)
    assert res["_agents_compared"] >= 2.0 and res["_factor_links_checked"] >= 1.0, res
    # flat ceilings on the raw figures next to the measured bars (what "noise" may mean)
    for k, cap in (("_trpo_kl_rel", 2e-2), ("_trpo_loss_rel", 1e-3), ("_trpo_dist_entropy_rel", 1e-4), ("_trpo_ratio_rel", 1e-3),
                   ("_trpo_step_size_rel", 2e-2), ("_trpo_expected_improve_rel", 2e-2), ("_factor_vec_rel_max", 1e-3),
                   ("_actor_final_param_vec_rel_max", 1e-2)):
        assert res[k] < cap, (k, res[k])


def test_humanoid17_full_size_against_oracle():
    """BASELINE configs[4] at the size `bench.py` measures it -- Humanoid-17x1, HATRPO, 17 agents x 204 800 rows (T = 200, 1024
    rollout threads), obs 393, MLP [128, 128, 128], CG 10 + line search -- against the oracle on identical buffer contents
    (gpu_checks.check_bench_config_parity_trpo): returns / generator state bit-exact; for agents 0, 1, 8 and 16 of the chain --
    each re-run by the oracle from the inputs the HIP path gave that step -- the same accept / reject decision and the same number
    of backtracks (integers), the five statistics, the step size, the final parameters and the factor handed to the next agent
    on measured bars; the critic 1e-5 flat."""
    res = _G().check_bench_config_parity_trpo("humanoid17", 1024, (0, 8, 16))
    print("humanoid17 full-size parity:", {k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in res.items()})
    _assert_trpo_full_size(res)


def test_hatrpo_gru128_full_size_against_oracle():
    """The coverage workload on the bench line -- HATRPO on hatrpo.yaml's default widths with a 128-wide GRU at the SMAC shape
    (8 agents x 81 920 rows, Discrete(14) with 30 % unavailable actions, chunks of 10): the composed per-step GRU and its
    forward-mode tangent at their measured size against the oracle's double backward; same assertions as the 17-agent check,
    the recurrent critic on the pooled bar."""
    res = _G().check_bench_config_parity_trpo("hatrpo_gru128", 512, (0, 7))
    print("hatrpo_gru128 full-size parity:", {k: (f"{v:.3e}" if isinstance(v, float) else v) for k, v in res.items()})
    _assert_trpo_full_size(res, tol=2e-5)  # (the recurrent fixtures' bar: nothing downstream of a GRU chain is held to 1e-5 flat)


def test_full_size_properties_baseline_config():
    """BASELINE configs[1] sizes (819 200 transitions x 3 agents): column independence vs the oracle, linearity of the
    unscaled sums under a column split, bit-exact determinism of train()."""
    res = _G().check_full_size_properties()
    for k, v in res.items():
        if "mismatch" in k or "count" in k:
            assert v == 0.0, (k, v)
        else:
            assert v < TOL, (k, v)


@pytest.mark.parametrize("name", ["mpe_disc_h64", "rnn_box_h64", "rnn_fp_box_h64_mb2"])
def test_buffer_generator_api_matches_reference_order(name):
    """Public *_generator_* methods of the buffers: same permutation draws, same gathered rows, reference tuple order."""
    for k, v in _G().check_generator_api(name).items():
        assert v == 0.0, (k, v)


@pytest.mark.parametrize("mode", ["hybrid", "1"])
@pytest.mark.parametrize("i", [0, 1])
def test_fused_update_kernels_single_update(i, mode, monkeypatch):
    """csrc/update.hip: forward + loss + head gradient in one launch, then either the layer-by-layer backward on the
    activation record of layer 1 that the launch leaves behind (HARL_FUSED_UPDATE=hybrid, the default) or the weight gradients
    from the recomputed x_hat_1 with transposes on the matrix pipe (=1) -- one actor and one critic update vs the oracle."""
    monkeypatch.setenv("HARL_FUSED_UPDATE", mode)
    G = _G()
    _assert_all(G.check_gradients(G.FWD_SHAPES[i]), tol=TOL)
    _assert_all(G.check_forward(G.FWD_SHAPES[i]), tol=TOL)


@pytest.mark.parametrize("mode", ["hybrid", "1", "logp"])
@pytest.mark.parametrize("name", ["mpe_box_h64", "mpe_box_h128", "mpe_disc_h64", "box_mean_inactive_novn", "a2c_box_h64",
                                  "mappo_box_h64", "cheetah_h128x3_mb2"])
def test_fused_update_kernels_train_golden(name, mode, monkeypatch):
    """Whole train() vs the reference's golden vectors with the optimiser steps routed through the fused forward + layer
    backward (hybrid, the default), the three fused launches (1) and the layer-by-layer kernels alone (logp)."""
    monkeypatch.setenv("HARL_FUSED_UPDATE", mode)
    _assert_all(_G().check_train_golden(name), tol=TOL)


@pytest.mark.parametrize("mode", ["0", "1", "auto"])
@pytest.mark.parametrize("name", ["mpe_box_h128", "cheetah_h128x3_mb2"])
def test_critic_stream_modes_train_golden(name, mode, monkeypatch):
    """Whole train() vs the reference's golden vectors with the critic's chain on the main stream (0), on a stream of its own (1)
    and under the size rule of round 6 (auto: own stream up to OnPolicyHARunner.CRITIC_STREAM_MAX_ROWS rows per minibatch)."""
    monkeypatch.setenv("HARL_CRITIC_STREAM", mode)
    _assert_all(_G().check_train_golden(name), tol=TOL)


@pytest.mark.parametrize("env", ["HARL_BWD_FUSED", "HARL_BWD_STREAMS"])
@pytest.mark.parametrize("name", ["mpe_box_h128", "cheetah_h128x3_mb2", "disc50_h128", "fp_disc_h128_mb2"])
def test_backward_variants_train_golden(name, env, monkeypatch):
    """Whole train() vs the reference's golden vectors with the two round-5 variants of the hidden layers' backward: the one-launch
    kernel (HARL_BWD_FUSED=1, harl_mlp_bwd_dx_dw) and the two-stream arrangement (HARL_BWD_STREAMS=1: weight gradients on a second
    stream next to the register-lean backward-dx launch)."""
    monkeypatch.setenv(env, "1")
    _assert_all(_G().check_train_golden(name), tol=TOL)


@pytest.mark.parametrize("i", range(4))
def test_trunk_in_one_launch_is_bit_identical(i):
    """harl_mlp_fwd_trunk / harl_mlp_bwd_trunk / harl_mlp_dw_partials_multi_v (round 6: a 64-wide trunk behind a wide first layer,
    with a fused GRU's input gates, in one launch per direction + one for every weight gradient) against the layer launches
    they replace: log-probs, values, gradients and stepped parameters of one actor and one critic update, bit for bit."""
    g = _G()
    _assert_all(g.check_trunk_fused(g.TRUNK_SPECS[i]))


@pytest.mark.parametrize("i", [0, 1])
def test_gate_weight_gradients_as_one_problem_bit_identical(i, monkeypatch):
    """harl_gru_dw6 (the six gate blocks of a GRU as one weight-gradient problem, every operand image read once; taken from
    160 000 rows per minibatch by default, forced here) inside the one-launch trunk path against the layer launches: the same bits."""
    monkeypatch.setenv("HARL_GRU_DW6", "1")
    g = _G()
    _assert_all(g.check_trunk_fused(g.TRUNK_SPECS[i]))


def test_gate_weight_gradients_on_a_second_stream_bit_identical(monkeypatch):
    """HARL_TRUNK_DW_STREAM=1 (opt-in: the six gate problems of harl_mlp_dw_partials_multi_v on a second stream next to
    harl_mlp_bwd_trunk, the MLP's problems behind it on the main one; no partial block is shared) inside the one-launch trunk path
    against the layer launches: the same bits."""
    monkeypatch.setenv("HARL_TRUNK_DW_STREAM", "1")
    g = _G()
    _assert_all(g.check_trunk_fused(g.TRUNK_SPECS[1]))


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("M", [45, 300, 32 * 4 * 7 + 1, 32 * 4 * 256 * 3 + 32 * 5 + 9])
def test_whole_layer_backward_in_one_launch(M, first):
    """harl_mlp_bwd_dx_dw (round 5: dx + dW' + db' + the fused first-layer gradient of a 128 x 128 layer in one launch) against a
    float64 restatement of autograd through Linear + ReLU + LayerNorm, and against the layer kernels it replaces; sizes from a
    single partial slab over a ragged super-round to several slabs per wave with a ragged tail; both filler modes."""
    G = _G()
    for fill in (1, 0):
        res = G.check_bwd_fused(M, first, fill=fill, seed=M % 97)
        for k, v in res.items():
            if "mismatch" in k:
                assert v == 0.0, (k, v, M, first, fill)
            else:
                assert v < 3e-6, (k, v, M, first, fill)


@pytest.mark.parametrize("mode", ["hybrid", "1"])
def test_fused_update_kernels_many_slabs_per_wave(mode):
    """The fused kernels against the layer-by-layer kernels at a size where every wave walks several slabs (the golden
    cases are a slab or two per wave): folded gradients, loss sums, log-probs and the factor product, plus bit-exact
    run-to-run determinism."""
    res = _G().check_fused_vs_layered(32 * 8 * 256 * 2 + 7 * 32 + 3, mode=mode)
    for k, v in res.items():
        if k.startswith("_"):
            continue
        if "bitwise" in k:
            assert v == 1.0, (k, v)
        else:
            assert v < 2e-5, (k, v)


@pytest.mark.parametrize("hidden,obs_dim", [((128, 128, 128), 23), ((64, 64, 64), 18), ((128, 128), 100)])
def test_last_layer_in_loss_launch_many_slabs_per_wave(hidden, obs_dim):
    """harl_update_last_* (the last hidden layer inside the loss launch: networks with three or more hidden layers, or a wide
    first layer) against the layer-by-layer kernels at a size where every wave walks several slabs: folded gradients, loss
    sums, log-probs, critic gradients; bit-exact run-to-run."""
    res = _G().check_fused_vs_layered(32 * 8 * 256 * 2 + 7 * 32 + 3, mode="hybrid", hidden=hidden, obs_dim=obs_dim)
    for k, v in res.items():
        if k.startswith("_"):
            continue
        if "bitwise" in k:
            assert v == 1.0, (k, v)
        else:
            assert v < 2e-5, (k, v)


@pytest.mark.parametrize("kind", ["width256", "multidiscrete"])
def test_many_slabs_per_wave_width256_and_multidiscrete(kind):
    """The 256-wide panel kernels (dexhands shape) and the MultiDiscrete head kernels (LAG layout) at sizes where every wave
    of the persistent kernels walks EIGHT or more slabs (their golden fixtures are a slab or two per wave):
    unscaled folded gradients and loss sums of the whole batch against the float64 sum over 8192-row chunks (linearity)."""
    G = _G()
    if kind == "width256":
        res = G.check_many_slabs_linearity(G.FWD_SHAPES[7], 32 * 8 * 1024 + 45)
    else:
        res = G.check_many_slabs_linearity(dict(name="md_lag_many", obs_dim=19, share_obs_dim=7, act_dim=153, discrete=True,
                                                hidden_sizes=[128, 128], nvec=[41, 41, 41, 30]), 32 * 8 * 2048 + 77)
    print(res)
    _assert_all(res, tol=2e-5)


@pytest.mark.parametrize("name", ["mpe3", "cheetah6", "smac3s5z", "humanoid17"])
def test_parity_at_baseline_shapes(name):
    """BASELINE.json configs 1-4 at their real network shapes, observation widths and FULL agent counts (thread count cut
    to <= 32 000 rows so the CPU oracle finishes): whole train() with one epoch per network vs the oracle."""
    _assert_all(_G().check_baseline_shape(name), tol=TOL)


def test_hatrpo_upstream_of_cg_at_humanoid_shape():
    """Humanoid-17x1 shape (obs 393, [128]x3, 17 agents), agents 0 / 8 / 16: surrogate gradient vector, F.v on three random
    vectors and the CG iterates after 1, 5, 10 steps, each against the oracle in float64 with the fp32 oracle's own distance
    next to it (printed).  Gradient and F.v are held to 1e-5 of the inf-norm, the CG iterates to 4 x the fp32 oracle's
    own distance from fp64; the figures without kink masking are reported, not asserted."""
    res = _G().check_trpo_upstream("humanoid17", (0, 8, 16))
    print({k: f"{v:.2e}" for k, v in res.items()})
    assert res["grad_vs_f64"] < 1e-5 and res["fvp_vs_f64"] < 1e-5, res
    for k in (1, 5, 10):
        assert res[f"cg{k}_excess"] <= 1.0, res


def test_run_with_eval_save_and_restore(tmp_path):
    """run(): eval() + save() every eval_interval episodes, restore() from train.model_dir in the constructor."""
    res = _G().check_run_eval_save_restore(str(tmp_path))
    for k, v in res.items():
        assert v == 0.0, (k, v)


def test_dropin_under_reference_launcher_on_gpu(tmp_path):
    """The unmodified examples/train.py with harl_amd installed under it, on the GPU (no stubs).  Needs a reference
    checkout next to the GPU (``HARL_REFERENCE``); skipped otherwise -- the CPU test tests/test_dropin_cpu.py covers the
    plumbing with recorded kernel calls where there is none."""
    import json
    import os
    import subprocess
    import sys
    ref = os.environ.get("HARL_REFERENCE", "/root/reference")
    if not os.path.exists(os.path.join(ref, "examples", "train.py")):
        pytest.skip("no reference checkout on this box")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "tests", "dropin_driver.py"), "--reference", ref, "--mode", "dropin",
           "--log-dir", str(tmp_path), "--algo", "happo", "--env", "pettingzoo_mpe", "--exp_name", "gpu", "--n_rollout_threads",
           "8", "--episode_length", "50", "--num_env_steps", "1600", "--eval_interval", "2", "--n_eval_rollout_threads", "2",
           "--eval_episodes", "2", "--log_interval", "1"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(os.environ, PYTHONPATH=root), cwd=root)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("DROPIN_RESULT ")][-1][len("DROPIN_RESULT "):])
    print("dropin on the GPU:", {k: res[k] for k in ("runner_class", "actor_class", "critic_class", "buffer_class", "saved") if k in res},
          "| last log lines:", [ln for ln in p.stdout.splitlines() if "reward" in ln.lower()][-2:])
    assert res["actor_class"] == "harl_amd.happo.HAPPO" and "critic_agent.pt" in res["saved"]


@pytest.mark.parametrize("case", ["ep_box", "ep_disc_avail", "fp_box", "fp_disc_avail"])
def test_buffer_slots_match_reference_insert_and_after_update(case):
    """A2 / B5: every slot of both buffers after T + 2 insert() calls around an after_update(), against the arrays the
    reference's own runner.insert() / buffer.after_update() produced from the same inputs (bit-exact)."""
    res = _G().check_buffer_slots(case)
    assert res["buffer_slot_mismatch"] == 0.0, res["_mismatched"]


def test_post_update_stream_leaves_every_figure_unchanged(monkeypatch):
    """Recurrent policies: the post-update log-prob pass on its own stream next to the following agent's first forward
    (runner.train, HARL_POST_STREAM) against the same update with everything on the main stream -- same kernels on the same
    operands, so every figure of the golden comparison must come out identical, not merely within tolerance."""
    G = _G()
    monkeypatch.setenv("HARL_POST_STREAM", "0")
    a = G.check_train_golden("rnn_disc_h64_mb2")
    monkeypatch.setenv("HARL_POST_STREAM", "1")
    b = G.check_train_golden("rnn_disc_h64_mb2")
    assert a == b, {k: (a[k], b.get(k)) for k in a if a[k] != b.get(k)}
