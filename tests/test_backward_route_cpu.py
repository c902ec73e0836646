"""The backward launch route of a network (nets._FlatNet._backward_route), host side without a GPU: its answers against the
conditions backward_trunk, _backward_trunk_fused and _ensure_ws used to state themselves -- quoted below as they stood before
the route was decided in one place -- over a sweep of networks and switch values, and the cached pointer arrays of the
one-launch trunk against the storage they point into."""
import itertools
import os

import pytest
import torch

from tests.gpu_checks import Box, Discrete, default_args
from tests.test_multidiscrete_cpu import stub_kernels  # noqa: F401  (fixture)

HIDDEN = ([128, 128], [128, 128, 128], [128, 64], [64, 64], [128], [256, 256])
IN_DIMS = (8, 32, 33, 64, 128)
# HARL_BWD_FUSED and the rows of the minibatch: unset below and above nets.BWD_FUSED_MIN_ROWS, then every value it takes
BWD_FUSED = ((None, 64), (None, 400_000), ("0", 64), ("1", 64), ("nofill", 64), ("fill", 64))
SWITCHES = ("HARL_BWD_FUSED", "HARL_BWD_K64", "HARL_BWD_STREAMS", "HARL_TRUNK_DW_STREAM", "HARL_GRU_DW6", "HARL_NWG",
            "HARL_TRUNK_FUSED", "HARL_GRU128", "HARL_GRU_COMPOSED")


def _networks():
    """(label, network) of the sweep: every combination a constructor accepts."""
    from harl_amd.nets import StochasticPolicy, VNet
    dev = torch.device("cpu")
    for hidden, in_dim, act, rnn in itertools.product(HIDDEN, IN_DIMS, ("relu", "tanh"), (False, True)):
        args = default_args(hidden, activation_func=act, use_recurrent_policy=rnn)
        for who, make in (("box3", lambda: StochasticPolicy(args, Box((in_dim,)), Box((3,)), dev)),
                          ("disc100", lambda: StochasticPolicy(args, Box((in_dim,)), Discrete(100), dev)),
                          ("critic", lambda: VNet(args, Box((in_dim,)), dev))):
            try:
                yield f"{hidden}/{in_dim}/{act}/{'gru' if rnn else 'ff'}/{who}", make()
            except NotImplementedError:
                pass


@pytest.fixture
def nets_(stub_kernels, monkeypatch):  # noqa: F811
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    torch.manual_seed(7)
    out = list(_networks())
    assert len(out) > 150
    return out


def _set(monkeypatch, **env):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


# ---- the conditions as the parent of this route stated them, literally (``self`` -> ``net``)
def _parent_cap(net, M):
    """_ensure_ws: "256 rows when every weight gradient of this network comes out of a one-workgroup-per-CU launch"."""
    from harl_amd.nets import _bwd_fused_mode
    self = net
    nwg_env = os.environ.get("HARL_NWG")
    return bool(not nwg_env and _bwd_fused_mode(M) == "1" and len(self.hidden_sizes) >= 2 and all(h == 128 for h in self.hidden_sizes)
                and ((self.in_dim + 31) // 32) * 32 == 32 and not (self.recurrent or self.grouped or self.act_id or self.panel))


def _parent_family(net):
    """backward_trunk's order of precedence."""
    self = net
    if self.trunk_fused() and not self.gru_wide:
        return "trunk"
    if self.panel:
        return "panel"
    if self.act_id:
        return "act"
    return "layers"


def _parent_layers(net, M, cuda):
    """backward_trunk's default layer loop: ({l: "full" | "side" | "plain"}, fill, where the first-layer gradient comes from)."""
    from harl_amd.nets import _bwd_fused_mode
    self = net
    L, kp0 = len(self.hidden_sizes), ((self.in_dim + 31) // 32) * 32
    has_x0n = self.in_dim <= 64 or self.wide  # (self.x0n is not None, _ensure_ws)
    fuse_dw1 = L >= 2 and has_x0n and self.in_dim < kp0 and kp0 <= 64
    bwd_mode = _bwd_fused_mode(M)
    if (bwd_mode != "0" and fuse_dw1 and kp0 == 64 and L >= 2 and self.hidden_sizes[0] == 128 and self.hidden_sizes[1] == 128
            and os.environ.get("HARL_BWD_K64", "0") == "1"):
        fuse_dw1 = False
    layers = {}
    for l in range(L - 1, 0, -1):
        ho, hi = self.hidden_sizes[l], self.hidden_sizes[l - 1]
        dw1_here = l == 1 and fuse_dw1
        if bwd_mode != "0" and ho == 128 and hi == 128 and (not dw1_here or kp0 == 32):
            layers[l] = "full"
            continue
        two = (os.environ.get("HARL_BWD_STREAMS", "0") == "1" and ho == 128 and hi == 128 and cuda
               and (not (l == 1 and fuse_dw1) or kp0 == 32))
        layers[l] = "side" if two else "plain"
    return layers, {"nofill": 0, "fill": 2}.get(bwd_mode, 1), "fused" if fuse_dw1 else "image" if has_x0n else "rows"


def _parent_trunk(net, M, cuda):
    """_backward_trunk_fused: (gate gradients on the second stream, gate gradients through harl_gru_dw6)."""
    self = net
    two = bool(self.recurrent and cuda and os.environ.get("HARL_TRUNK_DW_STREAM", "0") == "1")
    g6 = os.environ.get("HARL_GRU_DW6", "auto")
    return two, bool(self.recurrent and not two and (g6 == "1" or (g6 == "auto" and M >= 160000)))


def test_one_workgroup_per_cu_is_the_condition_ensure_ws_had(nets_, monkeypatch):
    seen = set()
    for mode, M in BWD_FUSED:
        _set(monkeypatch, HARL_BWD_FUSED=mode)
        for label, net in nets_:
            want = _parent_cap(net, M)
            assert net._backward_route(M).one_wg_per_cu is want, (label, mode, M)
            seen.add(want)
    assert seen == {True, False}


def test_route_is_what_the_backward_decided_inline(nets_, monkeypatch):
    families, firsts, launches = set(), set(), set()
    for (mode, M), k64, streams, cuda in itertools.product(BWD_FUSED, (None, "1"), (None, "1"), (False, True)):
        _set(monkeypatch, HARL_BWD_FUSED=mode, HARL_BWD_K64=k64, HARL_BWD_STREAMS=streams)
        for label, net in nets_:
            net.device_ = torch.device("cuda" if cuda else "cpu")
            r, what = net._backward_route(M), (label, mode, M, k64, streams, cuda)
            assert r.family == _parent_family(net), what
            assert r.gru == ("none" if not net.recurrent else "composed" if net.gru_wide else "fused"), what
            families.add((r.family, r.gru))
            if r.family != "layers":
                continue
            layers, fill, first = _parent_layers(net, M, cuda)
            assert {l: net._hidden_launch(r, l) for l in layers} == layers, what
            assert (r.fill, r.dw1) == (fill, first), what
            firsts.add(first)
            launches |= {(v, l == 1 and first == "fused") for l, v in layers.items()}
    assert families == {("trunk", "none"), ("trunk", "fused"), ("panel", "none"), ("act", "none"), ("layers", "none"),
                        ("layers", "fused"), ("layers", "composed")}
    assert firsts == {"fused", "image"}  # ("rows": inputs wider than 512, below)
    assert launches == {(k, f) for k in ("full", "side", "plain") for f in (True, False)}
    from harl_amd.nets import VNet
    wide = VNet(default_args([128, 128]), Box((520,)), torch.device("cpu"))
    assert wide._backward_route(64).dw1 == _parent_layers(wide, 64, False)[2] == "rows"


def test_second_streams_need_a_gpu_their_variable_and_a_layer_they_fit(nets_, monkeypatch):
    """The part of the two-stream arrangements a machine without a GPU can see: never on a CPU device; with the device type
    patched to "cuda", HARL_BWD_STREAMS puts exactly the 128 x 128 layers the layer kernels take on the second stream (not the
    one whose dx launch carries the first-layer gradient of a 64-wide image: the parent's ``not dw1_here or kp0 == 32``; none
    under the one-launch modes, which take those layers whole), HARL_TRUNK_DW_STREAM the gate blocks of a recurrent one-launch trunk."""
    on = dict(layers=0, trunk=0)
    for (mode, M), streams, tstream, g6, cuda in itertools.product(BWD_FUSED, (None, "0", "1"), (None, "0", "1"), (None, "0", "1"),
                                                                   (False, True)):
        _set(monkeypatch, HARL_BWD_FUSED=mode, HARL_BWD_STREAMS=streams, HARL_TRUNK_DW_STREAM=tstream, HARL_GRU_DW6=g6)
        for label, net in nets_:
            net.device_ = torch.device("cuda" if cuda else "cpu")
            r, what = net._backward_route(M), (label, mode, M, streams, tstream, g6, cuda)
            hs = net.hidden_sizes
            if r.family == "trunk":
                assert r.gates_side is (cuda and tstream == "1" and net.recurrent), what
                assert (r.gates_side, r.gates_dw6) == _parent_trunk(net, M, cuda), what
                on["trunk"] += r.gates_side
            else:
                assert not r.gates_side and not r.gates_dw6, what
            if r.family != "layers":
                continue
            layer_kernels = mode == "0" or (mode is None and M < 400_000)
            for l in range(1, len(hs)):
                carries64 = l == 1 and r.dw1 == "fused" and net.kp0 == 64
                want = cuda and streams == "1" and layer_kernels and hs[l] == 128 and hs[l - 1] == 128 and not carries64
                assert (net._hidden_launch(r, l) == "side") is want, what + (l,)
                on["layers"] += want
    assert all(on.values()), on


def test_switch_readers_are_what_graph_capture_asks(monkeypatch):
    """graphs.launches_capturable declines on the variable alone, whatever the network: the readers the route uses."""
    from harl_amd import configs, graphs
    for k in ("HARL_BWD_STREAMS", "HARL_TRUNK_DW_STREAM"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("HARL_GRAPH", "1")
    dev = torch.device("cuda")
    assert graphs.launches_capturable(dev) and not graphs.launches_capturable(torch.device("cpu"))
    for k, reader in (("HARL_BWD_STREAMS", configs.bwd_streams), ("HARL_TRUNK_DW_STREAM", configs.trunk_dw_stream)):
        for v, want in (("0", False), ("1", True)):
            monkeypatch.setenv(k, v)
            assert reader() is want and graphs.launches_capturable(dev) is (not want)
        monkeypatch.delenv(k)


def test_trunk_pointer_cache_follows_the_pack_arena(stub_kernels, monkeypatch):  # noqa: F811
    """_trunk_ptrs and the "bwd" entry of _trunk_cache hold raw addresses of pack_arena slices: a _build_tables() that gives
    pack_arena new storage must drop them, like _ensure_ws does for the workspaces (both through _new_addresses, which also
    bumps _ws_gen for the captured graphs)."""
    from harl_amd._lib import ptr
    from harl_amd.nets import VNet
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    calls, M, L = stub_kernels, 64, 3
    net = VNet(default_args([64] * L, use_recurrent_policy=True), Box((128,)), torch.device("cpu"))
    assert net._backward_route(M).family == "trunk"
    X = torch.randn(M, net.in_dim)
    seq = dict(L=4, m_pad=M // 4, h0=torch.zeros(M // 4, 64), mask_rows=torch.ones(M))

    def handed():
        """pW of harl_mlp_fwd_trunk and of harl_mlp_bwd_trunk, as the next forward and backward pass them."""
        calls.clear()
        net.forward_trunk(X, None, M, seq=seq)
        net.backward_trunk(X, None, M, seq=seq, head_dw_done=True)
        (fwd,), (bwd,) = calls["harl_mlp_fwd_trunk"], calls["harl_mlp_bwd_trunk"]
        return list(fwd[9]), list(bwd[8])

    def packs():
        return [ptr(net._packs[l][0]) for l in range(1, L)], [ptr(net._packs[l][0]) for l in range(L - 1, 0, -1)]

    net._ensure_ws(M)
    gen = net._ws_gen
    assert handed() == packs() and len(net._trunk_cache) == 2
    old = net.pack_arena  # (kept alive: the new arena cannot land on its address)
    net._build_tables()
    assert net.pack_arena.data_ptr() != old.data_ptr() and net._ws_gen == gen + 1
    assert handed() == packs()
