"""hipGraph replay of optimiser steps (opt-in: ``HARL_GRAPH=1``, default 0).

One optimiser step of a feed-forward actor or critic is a fixed chain of ten-odd launches whose arguments do not change
from step to step once the three per-step host scalars of the optimiser launch come from device memory
(``harl_adam_fold_dev``, nets.FusedAdam.begin_steps).  ``GraphedStep`` captures that chain once per (launch sequence, set of
device addresses) with ``torch.cuda.CUDAGraph`` and replays it for every later step: what a replay saves is the host's launch
path (Python + ctypes, ~3 us per launch), nothing on the device -- the kernels and the boundaries between them are the same.

Rules (README "Switches"):
  * a step is captured only after the identical launch sequence has run eagerly once in this process (the first call of a kernel
    with more than 64 KiB of LDS raises that limit -- csrc/common.h allow_big_lds -- which must not happen during capture);
  * one linear chain per graph: the region runs on ONE stream, no event, no second stream inside; waits on other streams are
    issued by the caller in front of the region, on the stream the graph is launched on;
  * the key of a graph is every device address the region reads or writes plus every host scalar that is baked into a launch;
    callers copy what used to be a fresh tensor per call into persistent buffers in front of the region;
  * a capture that fails is a Python exception: the capture is ended, the owner runs eagerly for the rest of the process
    (one warning), ``stats()`` shows it (``captures`` stays put, ``eager_steps`` grows).
"""
from __future__ import annotations

import os
import warnings
from typing import Callable, Dict, Hashable

import torch

from . import _lib
from .configs import bwd_streams, trunk_dw_stream

_capturing = False


def enabled() -> bool:
    return os.environ.get("HARL_GRAPH", "0") == "1"


def capturing() -> bool:
    """True while a GraphedStep records launches (nets._x0n_image refuses to launch inside: see there)."""
    return _capturing


def launches_capturable(device: torch.device) -> bool:
    """Graph mode is on, the device is a GPU, launches are not bracketed by timing events (bench.py's instrumented steps) and
    no variant that puts a second stream INSIDE an optimiser step is selected (the variable being set is enough, whatever the
    network: nets._backward_route decides per network)."""
    return (enabled() and device.type == "cuda" and not _lib._timing_on and not bwd_streams() and not trunk_dw_stream())


class GraphedStep:
    """The captured optimiser steps of ONE network (cache of graphs + counters)."""

    def __init__(self, name: str):
        self.name = name
        self._graphs: Dict[Hashable, torch.cuda.CUDAGraph] = {}
        self.warm: set = set()
        self._stream = None  # capture happens on a stream of its own (never the default stream); replays go to the caller's
        self.eager_only = False
        self.captures = self.replays = self.eager_steps = 0

    def stats(self) -> dict:
        return dict(captures=self.captures, replays=self.replays, eager_steps=self.eager_steps)

    def drop(self) -> None:
        """Forget the captured graphs (a workspace was reallocated, a table rebuilt, a buffer's storage changed)."""
        self._graphs.clear()

    def eager(self, fn: Callable[[], None]) -> None:
        self.eager_steps += 1
        fn()

    def run(self, warm_key: Hashable, key: Hashable, fn: Callable[[], None], opt) -> None:
        """One optimiser step: replay the graph of ``key``, or run ``fn`` eagerly (first time this launch sequence --
        ``warm_key`` -- is seen), or capture ``fn`` and replay the new graph once (capture does not execute anything).
        ``fn`` enqueues the step on torch's current stream and advances ``opt.step_count`` by one, nothing else on the host."""
        g = self._graphs.get(key)
        if g is not None:
            g.replay()
            opt.step_count += 1
            self.replays += 1
            return
        if self.eager_only or warm_key not in self.warm:
            self.eager(fn)
            self.warm.add(warm_key)
            return
        count = opt.step_count
        try:
            g = self._capture(fn)
        except Exception as e:  # a host sync or an unsupported call inside the region: a Python error, never a GPU fault
            opt.step_count = count
            self.eager_only = True
            self._graphs.clear()
            warnings.warn(f"HARL_GRAPH: capturing the optimiser step of {self.name} failed ({type(e).__name__}: {e}); "
                          "it runs eagerly for the rest of this process")
            self.eager(fn)
            return
        self._graphs[key] = g
        self.captures += 1
        g.replay()
        self.replays += 1

    def _capture(self, fn: Callable[[], None]) -> torch.cuda.CUDAGraph:
        global _capturing
        cur = torch.cuda.current_stream()
        if self._stream is None or self._stream.device != cur.device:
            self._stream = torch.cuda.Stream(device=cur.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(self._stream):
            g.capture_begin(capture_error_mode="thread_local")
            _capturing = True
            try:
                fn()
            except BaseException:
                _capturing = False
                try:
                    g.capture_end()
                except Exception:
                    pass
                raise
            _capturing = False
            g.capture_end()
        return g


def sum_stats(objs) -> dict:
    """Sum of ``graph_stats()`` over distinct objects (a shared actor counts once)."""
    out = dict(captures=0, replays=0, eager_steps=0)
    seen = []
    for o in objs:
        if any(o is s for s in seen) or not hasattr(o, "graph_stats"):
            continue
        seen.append(o)
        for k, v in o.graph_stats().items():
            out[k] += v
    return out
