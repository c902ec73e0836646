#!/usr/bin/env python3
"""Per-kernel micro-benchmark through the C ABI at the bench shape (B = 200*4096 samples, H = 128).

    python tools/kbench.py [--reps 20] [--lib path/to/libharl_hip.so] [filter ...]

Prints ms per launch and the algorithmic TFLOP/s or TB/s of each kernel (HIP events on the launch stream)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--B", type=int, default=200 * 4096)
    ap.add_argument("filters", nargs="*")
    args = ap.parse_args()
    from harl_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    from harl_amd._lib import call, ptr, stream
    dev = torch.device("cuda:0")
    B, H = args.B, 128
    ns = (B + 31) // 32
    mp = ns * 32
    g = torch.Generator(device=dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    obs, sobs = rn(B, 18), rn(B, 54)
    xh1, xh2, dz, dz2 = rn(mp * H), rn(mp * H), rn(mp * H), torch.empty(mp * H, device=dev)
    mask = torch.randint(-2**31, 2**31 - 1, (ns * 2 * 64,), device=dev, dtype=torch.int32, generator=g)
    rstd = torch.rand(mp, device=dev, generator=g) + 0.5
    mu0, rstd0 = torch.zeros(mp, device=dev), torch.ones(mp, device=dev)
    W = rn(H * H) * 0.1
    b = rn(H) * 0.1
    W1, W1c = rn(H * 18) * 0.2, rn(H * 54) * 0.2
    Wh, bh, ls = rn(5 * H) * 0.05, rn(5) * 0.1, torch.ones(5, device=dev)
    Wv, bv = rn(H) * 0.05, rn(1)
    actions, old_logp = rn(B, 5), rn(B, 5) * 0.1 - 1
    adv, factor, active = rn(B), torch.ones(B, device=dev), torch.ones(B, device=dev)
    dhead = rn(mp * 32) * 0.01
    n_wg = 512
    part = torch.empty(n_wg * (H * H + H), device=dev)
    dwp = torch.empty(H * H + H, device=dev)
    nb = _lib.load().harl_head_blocks(B)
    ps = torch.zeros(nb * 48, device=dev)
    logp_out = torch.empty(B, 5, device=dev)
    vals = torch.empty(B, device=dev)
    vp, ret = rn(B), rn(B)
    vn = torch.tensor([0.1, 1.2, 0.9], device=dev)
    T, N = 200, B // 200
    rew, vpT, mk = rn(T, N), rn(T + 1, N), (torch.rand(T + 1, N, device=dev) > 0.04).float()
    rets, advs = torch.empty(T + 1, N, device=dev), torch.empty(T, N, device=dev)
    P = 20142
    pp, gg, mm, vv = rn(P), rn(P), torch.zeros(P, device=dev), torch.zeros(P, device=dev)
    x0n32 = rn(mp * 32)
    x0n64 = rn(mp * 64)
    wimg = torch.empty(3 * H * 64 // 2, device=dev)
    ps_f = torch.zeros(n_wg * 48, device=dev)
    part_h = torch.empty(n_wg * (32 * H + 32), device=dev)
    part_1 = torch.empty(n_wg * (H * 32 + H), device=dev)
    s = stream()
    # the MPE update's head: three actors' observations and the critic's, each with buffers of its own, in ONE launch
    multi_bufs = [(rn(B, 18), torch.empty(mp * 32, device=dev), torch.empty(mp, device=dev), torch.empty(mp, device=dev)) for _ in range(3)]
    multi_bufs.append((rn(B, 54), torch.empty(mp * 64, device=dev), torch.empty(mp, device=dev), torch.empty(mp, device=dev)))
    multi_problems = [(ptr(x), x.shape[1], B, x.shape[1], 1, ptr(im), ptr(mu), ptr(rs)) for x, im, mu, rs in multi_bufs]
    GF = lambda f: ("TFLOP/s", f / 1e12)  # noqa: E731
    GB = lambda f: ("TB/s", f / 1e12)  # noqa: E731
    fl = 2.0 * B * H * H
    jobs = [
        ("fwd_input_D18", lambda: call("harl_mlp_fwd_input", ptr(obs), 18, None, B, 18, ptr(W1), ptr(b), 1, H, ptr(xh1), ptr(mask), ptr(rstd), ptr(mu0), ptr(rstd0), None, s), GB(B * (72 + 512 + 20))),
        ("fwd_input_D54", lambda: call("harl_mlp_fwd_input", ptr(sobs), 54, None, B, 54, ptr(W1c), ptr(b), 1, H, ptr(xh1), ptr(mask), ptr(rstd), ptr(mu0), ptr(rstd0), None, s), GB(B * (216 + 512 + 20))),
        ("fwd_fused2_D18_train", lambda: call("harl_mlp_fwd_fused2", ptr(obs), 18, None, B, 18, ptr(W1), ptr(b), 1, ptr(W), ptr(b), H, 1, ptr(xh1), ptr(mask), ptr(rstd), ptr(mu0), ptr(rstd0), ptr(xh2), ptr(mask), ptr(rstd), None, s), GF(fl + 2.0 * B * 18 * H)),
        ("fwd_fused2_D18_logp", lambda: call("harl_mlp_fwd_fused2", ptr(obs), 18, None, B, 18, ptr(W1), ptr(b), 1, ptr(W), ptr(b), H, 0, ptr(xh1), ptr(mask), ptr(rstd), ptr(mu0), ptr(rstd0), ptr(xh2), ptr(mask), ptr(rstd), None, s), GF(fl + 2.0 * B * 18 * H)),
        ("x0n_D18", lambda: call("harl_mlp_x0n_wide", ptr(obs), 18, None, B, 18, 1, ptr(x0n32), ptr(mu0), ptr(rstd0), s), GB(B * (72 + 128 + 8))),
        ("x0n_D54", lambda: call("harl_mlp_x0n_wide", ptr(sobs), 54, None, B, 54, 1, ptr(x0n64), ptr(mu0), ptr(rstd0), s), GB(B * (216 + 256 + 8))),
        ("x0n_multi_mpe", lambda: _lib.x0n_multi(multi_problems, tag=None), GB(B * (3 * (72 + 128 + 8) + 216 + 256 + 8))),
        ("fwd_fused2x_train", lambda: call("harl_mlp_fwd_fused2x", ptr(x0n32), B, ptr(W1), 18, ptr(b), ptr(W), ptr(b), H, 1, ptr(xh1), ptr(mask), ptr(rstd), ptr(xh2), ptr(mask), ptr(rstd), s), GF(fl + 2.0 * B * 18 * H)),
        ("fwd_fused2x_logp", lambda: call("harl_mlp_fwd_fused2x", ptr(x0n32), B, ptr(W1), 18, ptr(b), ptr(W), ptr(b), H, 0, ptr(xh1), ptr(mask), ptr(rstd), ptr(xh2), ptr(mask), ptr(rstd), s), GF(fl + 2.0 * B * 18 * H)),
        ("fwd_wide_K64", lambda: call("harl_mlp_fwd_wide", ptr(x0n64), B, 64, ptr(W1c), 54, ptr(b), H, ptr(wimg), ptr(xh1), ptr(mask), ptr(rstd), s), GB(B * (256 + 512 + 20))),
        ("fwd_hidden", lambda: call("harl_mlp_fwd_hidden", ptr(xh1), B, H, H, ptr(W), ptr(b), ptr(xh2), ptr(mask), ptr(rstd), s), GF(fl)),
        ("bwd_dx", lambda: call("harl_mlp_bwd_dx", ptr(dz), ptr(xh1), ptr(mask), ptr(rstd), B, H, H, ptr(W), ptr(dz2), None, 0, None, 0, s), GF(fl)),
        ("bwd_full_fill", lambda: call("harl_mlp_bwd_dx_dw", ptr(dz), ptr(xh1), ptr(mask), ptr(rstd), B, H, H, ptr(W), ptr(dz2), None, 0, None, ptr(part), n_wg, 2, s), GF(2 * fl)),
        ("bwd_full_nofill", lambda: call("harl_mlp_bwd_dx_dw", ptr(dz), ptr(xh1), ptr(mask), ptr(rstd), B, H, H, ptr(W), ptr(dz2), None, 0, None, ptr(part), n_wg, 0, s), GF(2 * fl)),
        ("bwd_full_dw1_fill", lambda: call("harl_mlp_bwd_dx_dw", ptr(dz), ptr(xh1), ptr(mask), ptr(rstd), B, H, H, ptr(W), None, ptr(x0n32), 32, ptr(part_1), ptr(part), n_wg, 2, s), GF(2 * fl + 2.0 * B * H * 18)),
        ("bwd_full_dw1_nofill", lambda: call("harl_mlp_bwd_dx_dw", ptr(dz), ptr(xh1), ptr(mask), ptr(rstd), B, H, H, ptr(W), None, ptr(x0n32), 32, ptr(part_1), ptr(part), n_wg, 0, s), GF(2 * fl + 2.0 * B * H * 18)),
        ("bwd_dx_dw1_fused", lambda: call("harl_mlp_bwd_dx", ptr(dz), ptr(xh1), ptr(mask), ptr(rstd), B, H, H, ptr(W), None, ptr(x0n32), 32, ptr(part_1), n_wg, s), GF(fl + 2.0 * B * H * 18)),
        ("dw_hidden", lambda: call("harl_mlp_dw_partials", ptr(dz), 0, 0, H, ptr(xh1), 0, 0, None, None, None, H, B, ptr(part), n_wg, s), GF(fl)),
        ("dw_head", lambda: call("harl_mlp_dw_partials", ptr(dhead), 1, 32, 5, ptr(xh2), 0, 0, None, None, None, H, B, ptr(part), n_wg, s), GB(B * (512 + 128))),
        ("dw_input_D18", lambda: call("harl_mlp_dw_partials", ptr(dz), 0, 0, H, ptr(obs), 1, 18, None, ptr(mu0), ptr(rstd0), 18, B, ptr(part), n_wg, s), GB(B * (512 + 72 + 8))),
        ("dw_input_atl32", lambda: call("harl_mlp_dw_partials", ptr(dz), 0, 0, H, ptr(xh1), 0, 0, None, None, None, 32, B, ptr(part), n_wg, s), GB(B * (512 + 128))),
        ("dw_input_atl64", lambda: call("harl_mlp_dw_partials", ptr(dz), 0, 0, H, ptr(xh1), 0, 0, None, None, None, 64, B, ptr(part), n_wg, s), GB(B * (512 + 256))),
        ("dw_input_D54", lambda: call("harl_mlp_dw_partials", ptr(dz), 0, 0, H, ptr(sobs), 1, 54, None, ptr(mu0), ptr(rstd0), 54, B, ptr(part), n_wg, s), GB(B * (512 + 216 + 8))),
        ("reduce_partials", lambda: call("harl_reduce_partials", ptr(part), n_wg, H * H + H, ptr(dwp), s), GB(n_wg * (H * H + H) * 4)),
        ("actor_head_logp", lambda: call("harl_actor_head_logp", ptr(xh2), B, H, ptr(Wh), ptr(bh), ptr(ls), 1.0, 0.5, 0, 5, ptr(actions), None, ptr(logp_out), None, None, 0, None, 0, 0, s), GB(B * (512 + 40))),
        ("actor_head_loss", lambda: call("harl_actor_head_loss", ptr(xh2), ptr(mask), ptr(rstd), B, H, ptr(Wh), ptr(bh), ptr(ls), 1.0, 0.5, 0, 5, None, ptr(actions), None, ptr(old_logp), ptr(adv), None, ptr(factor), ptr(active), 0.2, 0.01, 0, 0, 0, 0, None, ptr(dz2), ptr(dhead), ptr(ps), None, 0, s), GB(B * (512 + 512 + 128 + 60))),
        ("actor_head_loss_fused_dw", lambda: call("harl_actor_head_loss", ptr(xh2), ptr(mask), ptr(rstd), B, H, ptr(Wh), ptr(bh), ptr(ls), 1.0, 0.5, 0, 5, None, ptr(actions), None, ptr(old_logp), ptr(adv), None, ptr(factor), ptr(active), 0.2, 0.01, 0, 0, 0, 0, None, ptr(dz2), None, ptr(ps_f), ptr(part_h), n_wg, s), GB(B * (512 + 512 + 20 + 60))),
        ("critic_head_loss_fused_dw", lambda: call("harl_critic_head_loss", ptr(xh2), ptr(mask), ptr(rstd), B, H, ptr(Wv), ptr(bv), None, ptr(vp), ptr(ret), ptr(vn), 0.2, 1, 1, 10.0, 0, 0, ptr(dz2), None, ptr(ps_f), ptr(part_h), n_wg, s), GB(B * (512 + 512 + 20 + 8))),
        ("critic_head_loss", lambda: call("harl_critic_head_loss", ptr(xh2), ptr(mask), ptr(rstd), B, H, ptr(Wv), ptr(bv), None, ptr(vp), ptr(ret), ptr(vn), 0.2, 1, 1, 10.0, 0, 0, ptr(dz2), ptr(dhead), ptr(ps), None, 0, s), GB(B * (512 + 512 + 128 + 8))),
        ("critic_head_values", lambda: call("harl_critic_head_values", ptr(xh2), B, H, ptr(Wv), ptr(bv), ptr(vals), s), GB(B * 516)),
        ("gae_returns", lambda: call("harl_gae_returns", ptr(rew), ptr(vpT), ptr(mk), ptr(mk), ptr(vpT[-1].contiguous()), ptr(vn), ptr(rets), ptr(advs), T, N, 0.99, 0.9405, 1, 1, 0, s), GB(B * 24)),
        ("gradnorm_clip_adam", lambda: call("harl_gradnorm_clip_adam", ptr(pp), ptr(gg), ptr(mm), ptr(vv), P, None, 1, 10.0, 5e-4, 0.9, 0.999, 1e-5, 0.0, 0.1, 0.001, None, s), GB(P * 28)),
    ]
    # ---- the 17-agent HATRPO shape (204 800 rows per launch, obs 393 -> KP 416): tangent / wide-input kernels of the FVP
    B2 = 200 * 1024
    ns2 = (B2 + 31) // 32
    mp2 = ns2 * 32
    x0n416 = rn(mp2 * 416)
    W1h, W1hd = rn(H * 393) * 0.05, rn(H * 393) * 0.05
    wimg416 = torch.empty(3 * H * 416 // 2, device=dev)
    timg = torch.empty(3 * H * H, device=dev)
    xa, xb, xc, xo = rn(mp2 * H), rn(mp2 * H), rn(mp2 * H), torch.empty(mp2 * H, device=dev)
    Wd = rn(H * H) * 0.1
    mask2_, rstd2_ = mask[:ns2 * 2 * 64], rstd[:mp2]
    fl2 = 2.0 * B2 * H * H
    jobs += [
        ("h17_fwd_wide_K416", lambda: call("harl_mlp_fwd_wide", ptr(x0n416), B2, 416, ptr(W1h), 393, ptr(b), H, ptr(wimg416), ptr(xo), ptr(mask2_), ptr(rstd2_), s), GB(B2 * (1664 + 512 + 20))),
        ("h17_tangent_wide_K416", lambda: call("harl_mlp_tangent_wide", ptr(x0n416), B2, 416, ptr(W1hd), 393, ptr(b), H, ptr(wimg416), ptr(xa), ptr(mask2_), ptr(rstd2_), ptr(xo), s), GB(B2 * (1664 + 512 + 512 + 20))),
        ("h17_tangent_hidden2", lambda: call("harl_mlp_tangent_hidden2", ptr(xb), ptr(xa), B2, H, H, ptr(W), ptr(Wd), ptr(b), ptr(timg), ptr(xc), ptr(mask2_), ptr(rstd2_), ptr(xo), s), GB(B2 * (512 * 4 + 20))),
        ("h17_fwd_hidden", lambda: call("harl_mlp_fwd_hidden", ptr(xa), B2, H, H, ptr(W), ptr(b), ptr(xo), ptr(mask2_), ptr(rstd2_), s), GB(B2 * (1024 + 20))),
        ("h17_bwd_dx", lambda: call("harl_mlp_bwd_dx", ptr(xa), ptr(xb), ptr(mask2_), ptr(rstd2_), B2, H, H, ptr(W), ptr(xo), None, 0, None, 0, s), GB(B2 * (1536 + 20))),
        ("h17_dw_hidden", lambda: call("harl_mlp_dw_partials", ptr(xa), 0, 0, H, ptr(xb), 0, 0, None, None, None, H, B2, ptr(part), n_wg, s), GB(B2 * 1024)),
    ]
    # ---- the same rows on layers with a 256-wide side: the tangent of a rectangular pair (k_panel_rect<MT, 2>, one stream of
    # sub-panels) next to k_panel<2> (one walk per operand) at 256 -> 256, the one shape both take
    ya, yb, yc, yo = rn(mp2 * 256), rn(mp2 * 256), rn(mp2 * 256), torch.empty(mp2 * 256, device=dev)
    Wr, Wrd, br = rn(256 * 256) * 0.06, rn(256 * 256) * 0.06, rn(256) * 0.1
    mask4_ = mask[:ns2 * 4 * 64]
    rect = lambda hi, ho: lambda: call("harl_mlp_rect_tangent", ptr(yb), ptr(ya), B2, hi, ho, ptr(Wr), ptr(Wrd), hi, ptr(br), ptr(yc), ptr(mask4_), ptr(rstd2_), ptr(yo), s)  # noqa: E731
    jobs += [
        ("h17_tangent_rect_256to128", rect(256, 128), GF(2 * 2.0 * B2 * 256 * 128)),
        ("h17_tangent_rect_128to256", rect(128, 256), GF(2 * 2.0 * B2 * 128 * 256)),
        ("h17_tangent_rect_256to256", rect(256, 256), GF(2 * 2.0 * B2 * 256 * 256)),
        ("h17_tangent_panel_256to256", lambda: call("harl_mlp_panel_tangent", ptr(yb), ptr(ya), B2, 256, ptr(Wr), ptr(Wrd), 256, ptr(br), ptr(yc), ptr(mask4_), ptr(rstd2_), ptr(yo), s), GF(2 * 2.0 * B2 * 256 * 256)),
    ]
    # ---- a Categorical head of 512 actions (four groups of 128 rows) on a 128-wide head input, the same rows: the grouped
    # launches of csrc/rect.hip (HARL_CAT_WIDE_256=1) next to the launches they stand in for on trunks that hold a 256-wide layer
    import ctypes as C
    zg = [rn(mp2 * H) for _ in range(4)]
    Wg, bg = [rn(H * H) * 0.1 for _ in range(4)], [rn(H) * 0.1 for _ in range(4)]
    arr = lambda ts: (C.c_void_p * 4)(*[t.data_ptr() for t in ts])  # noqa: E731
    sp4, zs4, Ws4, bs4 = (C.c_int * 4)(*[H] * 4), arr(zg), arr(Wg), arr(bg)

    def four_linear():
        for g_ in range(4):
            call("harl_mlp_linear", ptr(xa), B2, H, H, ptr(Wg[g_]), ptr(bg[g_]), ptr(zg[g_]), s)

    def four_bwd_dx():
        for g_ in range(4):
            call("harl_mlp_bwd_dx", ptr(zg[g_]), ptr(xb), ptr(mask2_), ptr(rstd2_), B2, H, H, ptr(Wg[g_]), ptr(xo if g_ == 0 else xc), None, 0, None, 0, s)
            if g_:
                xo.add_(xc)

    jobs += [
        ("h17_cat512_linear_groups", lambda: call("harl_mlp_rect_linear_groups", ptr(xa), B2, H, 4, sp4, Ws4, bs4, zs4, s), GF(4 * fl2)),
        ("h17_cat512_linear_x4", four_linear, GF(4 * fl2)),
        ("h17_cat512_bwd_groups", lambda: call("harl_mlp_rect_bwd_groups", zs4, 4, sp4, Ws4, ptr(xb), ptr(mask2_), ptr(rstd2_), B2, H, ptr(xo), s), GF(4 * fl2)),
        ("h17_cat512_bwd_dx_x4_add", four_bwd_dx, GF(4 * fl2)),
    ]
    # ---- the tangent of those logits (HARL_TRPO_CAT_WIDE_256=1): one launch into one image per group next to the 2 G
    # harl_mlp_linear launches into two images per group of the 64 / 128-wide trunks; then the 256-wide head input, which has no
    # other kernel
    zg2, Wgd, zb128 = [torch.empty(mp2 * H, device=dev) for _ in range(4)], [rn(H * H) * 0.1 for _ in range(4)], torch.zeros(H, device=dev)
    Wg256, Wgd256 = [rn(H * 256) * 0.06 for _ in range(4)], [rn(H * 256) * 0.06 for _ in range(4)]
    Wds4, Ws256, Wds256 = arr(Wgd), arr(Wg256), arr(Wgd256)

    def eight_linear():
        for g_ in range(4):
            call("harl_mlp_linear", ptr(xb), B2, H, H, ptr(Wg[g_]), ptr(zb128), ptr(zg[g_]), s)
            call("harl_mlp_linear", ptr(xa), B2, H, H, ptr(Wgd[g_]), ptr(bg[g_]), ptr(zg2[g_]), s)

    jobs += [
        ("h17_cat512_tangent_groups", lambda: call("harl_mlp_rect_tangent_groups", ptr(xb), ptr(xa), B2, H, 4, sp4, Ws4, Wds4, bs4, zs4, s), GF(8 * fl2)),
        ("h17_cat512_linear_x8", eight_linear, GF(8 * fl2)),
        ("h17_cat512_tangent_groups_K256", lambda: call("harl_mlp_rect_tangent_groups", ptr(yb), ptr(ya), B2, 256, 4, sp4, Ws256, Wds256, bs4, zs4, s), GF(16 * fl2)),
    ]
    # ---- HARL_ACT_256=1: k_panel_rect<MT, MODE, ACT> with the tanh epilogue next to the ReLU launch of the same shape and rows
    # (filter "rect_relu" with --lib on another build: the yardstick of profiles/r21_act_256.md)
    rstd_o, mean_o = torch.empty(mp2, device=dev), torch.zeros(mp2, device=dev)
    for hi, ho in ((256, 128), (128, 256), (256, 256)):
        f = GF(2.0 * B2 * hi * ho)
        jobs += [
            (f"h17_rect_relu_fwd_{hi}to{ho}", lambda hi=hi, ho=ho: call("harl_mlp_rect_fwd", ptr(ya), B2, hi, ptr(Wr), hi, ptr(br), ho, ptr(yo), ptr(mask4_), ptr(rstd_o), s), f),
            (f"h17_rect_tanh_fwd_{hi}to{ho}", lambda hi=hi, ho=ho: call("harl_mlp_rect_act_fwd", ptr(ya), B2, hi, ptr(Wr), hi, ptr(br), ho, 2, ptr(yo), ptr(mean_o), ptr(rstd_o), s), f),
            (f"h17_rect_relu_bwd_{ho}to{hi}", lambda hi=hi, ho=ho: call("harl_mlp_rect_bwd", ptr(yb), ptr(ya), ptr(mask4_), ptr(rstd2_), B2, ho, hi, ptr(Wr), ptr(yo), s), f),
            (f"h17_rect_tanh_bwd_{ho}to{hi}", lambda hi=hi, ho=ho: call("harl_mlp_rect_act_bwd", ptr(yb), ptr(ya), ptr(mean_o), ptr(rstd2_), B2, ho, hi, 2, ptr(Wr), ptr(yo), s), f),
        ]
    # ---- HARL_TRPO_ACT_256=1: k_panel_rect<MT, 2, ACT> with the tanh slope in its epilogue; the ReLU tangent of the same shape and
    # rows is h17_tangent_rect_* above (filter "tangent_rect_2" with --lib on another build: the yardstick of
    # profiles/r22_trpo_act_256.md)
    for hi, ho in ((256, 128), (256, 256)):
        jobs.append((f"h17_tangent_rect_tanh_{hi}to{ho}", lambda hi=hi, ho=ho: call(
            "harl_mlp_rect_act_tangent", ptr(yb), ptr(ya), B2, hi, ho, ptr(Wr), ptr(Wrd), hi, ptr(br), 2, ptr(yc), ptr(mean_o), ptr(rstd2_),
            ptr(yo), s), GF(2 * 2.0 * B2 * hi * ho)))
    # ---- HARL_HEAD64_256=1: plain heads of 33 and 64 outputs on a 256-wide head input (k_head256, csrc/head256.hip) -- log-prob
    # pass, loss + backward, and the head's weight gradient from the ATL(64) dhead image -- next to the 32-output head of
    # csrc/heads.hip on the same rows (the yardstick of profiles/r23_head64_256.md)
    nb2 = _lib.load().harl_head_blocks(B2)
    ps2, pls2 = torch.zeros(nb2 * 48, device=dev), torch.zeros(nb2 * 64, device=dev)
    Wh256, bh64, ls64 = rn(64 * 256) * 0.05, rn(64) * 0.1, torch.ones(64, device=dev)
    dhead64, lp64 = torch.empty(mp2 * 64, device=dev), torch.empty(B2 * 64, device=dev)
    adv2, one2 = adv[:B2].contiguous(), factor[:B2].contiguous()
    for disc, nm in ((1, "cat"), (0, "box")):
        for D in (32, 33, 64):
            act_ = torch.randint(0, D, (B2,), device=dev, generator=g).float() if disc else rn(B2, D)
            olp_ = rn(B2, 1 if disc else D) * 0.1 - 1
            loss_fn = "harl_actor_head_loss" if (disc or D <= 32) else "harl_actor_head_loss_ls"
            tail = (s,) if loss_fn == "harl_actor_head_loss" else (ptr(pls2), s)
            byt = GB(B2 * (1024 + 1024 + 20 + 4 * (64 if D > 32 else 32) + 4 * (2 if disc else 2 * D)))
            jobs += [
                (f"h256_{nm}{D}_logp", lambda disc=disc, D=D, act_=act_: call(
                    "harl_actor_head_logp", ptr(ya), B2, 256, ptr(Wh256), ptr(bh64), ptr(ls64), 1.0, 0.5, disc, D, ptr(act_), None, ptr(lp64),
                    None, None, 0, None, 0, 0, s), GB(B2 * (1024 + 4 * (2 if disc else 2 * D)))),
                (f"h256_{nm}{D}_loss", lambda disc=disc, D=D, act_=act_, olp_=olp_, loss_fn=loss_fn, tail=tail: call(
                    loss_fn, ptr(ya), ptr(mask4_), ptr(rstd2_), B2, 256, ptr(Wh256), ptr(bh64), ptr(ls64), 1.0, 0.5, disc, D, None, ptr(act_),
                    None, ptr(olp_), ptr(adv2), None, ptr(one2), ptr(one2), 0.2, 0.01, 0, 0, 0, 0, None, ptr(yo), ptr(dhead64), ptr(ps2),
                    None, 0, *tail), byt),
            ]
            if D == 64 and disc:  # (the same launch for both kinds of head and every width above 32)
                jobs.append(("h256_dw_head_atl64", lambda: call("harl_mlp_dw_partials", ptr(dhead64), 0, 0, 64, ptr(ya), 0, 0, None, None,
                                                                     None, 256, B2, ptr(part), n_wg, s), GB(B2 * (1024 + 256))))
    # ---- HARL_TRPO_HEAD64_256=1: the head part of HATRPO's Fisher-vector product on the same rows -- 33 and 64 actions on
    # k_head256_fvp (csrc/head256.hip), 32 on k_actor_head_fvp<256, 32, true> (csrc/heads.hip), the nearest existing kernel; the
    # training pass of k_head256 is h256_cat*_loss above (profiles/r24_trpo_head64_256.md)
    Whd256, bhd64 = rn(64 * 256) * 0.05, rn(64) * 0.1
    for D in (32, 33, 64):
        jobs.append((f"h256_cat{D}_fvp", lambda D=D: call(
            "harl_actor_head_fvp", ptr(ya), ptr(yb), ptr(mask4_), ptr(rstd2_), B2, 256, ptr(Wh256), ptr(bh64), ptr(Whd256), ptr(bhd64),
            None, 1.0, 0.5, 1, D, None, 0, 0, ptr(yo), ptr(dhead64), s), GB(B2 * (3 * 1024 + 20 + 4 * (64 if D > 32 else 32)))))
    print(f"B={B}  H={H}  reps={args.reps}  lib={_lib.LIB_PATH}")
    for name, fn, (unit, work) in jobs:
        if args.filters and not any(f in name for f in args.filters):
            continue
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        evs = []
        for _ in range(args.reps):
            a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b_.record()
            evs.append((a, b_))
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b_) for a, b_ in evs)
        med, mn = ms[len(ms) // 2], ms[0]
        print(f"{name:22s} median {med:8.4f} ms  min {mn:8.4f} ms   {work / (med * 1e-3):8.2f} {unit}")


if __name__ == "__main__":
    main()
