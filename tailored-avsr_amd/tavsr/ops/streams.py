"""Which queue a launch goes to, and what orders the queues: fork / join scopes (``BranchScope``), weight gradients left in
flight beside the backward chain (``wgrad_*``) and the race amplifier of the tests (``arm_race_probe``).

Stream safety.  The package runs independent sections on forked HIP streams (``BranchScope``; autograd replays a node on the stream
its forward ran on).  Two rules make that safe against torch's per-stream caching allocator.  Both are enforced in ``_lib.py``, at the
one place where a tensor becomes a raw pointer (``ptr`` / ``addr``) and at the head of every autograd backward (``enter_node``),
instead of by hand at the fork sites:
  1. a tensor handed to a launch on a forked stream is ``record_stream``-ed on it (a no-op for tensors of that stream's own
     pool): the allocator will not hand its block to anybody before the forked stream has passed the point of the free;
  2. a forked stream never starts work without first waiting for the stream that owns it (``BranchScope.__enter__``,
     ``enter_node``): blocks of the forked stream's pool are only re-used behind every reader the owning stream had enqueued
     when they were freed.
What this file adds to them: every side stream is registered with its owner (``branch_stream``), a scope tells ``_lib`` where
launches go (``push_fork`` / ``pop_fork``), and launches that C code enqueues on a side queue itself - no ``ptr`` call sees them -
get rule 1 by hand from their caller (``blocks.conv2d_subsample_bwd``).  ``tests/test_host_api.py`` checks that no module takes a
tensor's address behind ``_lib``'s back.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from .. import _lib as L
from .. import ops
from .._lib import check, lib, stream

__all__ = ["forks_enabled", "branch_stream", "own_stream", "spin", "arm_race_probe", "BranchScope", "wgrad_fence", "wgrad_may_go_beside",
           "wgrad_open", "wgrad_beside", "branch_events"]


# The two Branchformer branches (attention | cgMLP) are independent between the fork after the macaron FFN and the
# merge: the attention branch is a chain of small latency-bound launches that fits beside the cgMLP GEMMs.


_BRANCH = {}


def forks_enabled() -> bool:
    """TAVSR_SINGLE_STREAM=1 (or ``_lib.SINGLE_STREAM = True`` at run time) puts every launch of the package on the calling
    stream - the reference's queueing; results must not depend on it (tests/test_gpu_streams.py)."""
    return not L.SINGLE_STREAM


def branch_stream(main: torch.cuda.Stream, slot: int = 0) -> torch.cuda.Stream:
    """the side stream that belongs to ``main`` (one per forking stream and ``slot``, so nested forks never share a stream with
    their siblings; ``slot`` > 0: a further side stream of the same owner, for a second section that runs beside the first)."""
    key = (main.device.index, main.cuda_stream, slot)
    s = _BRANCH.get(key)
    if s is None:
        s = _BRANCH[key] = own_stream(main.device)
        L.register_fork(s, main)
    return s


def own_stream(device) -> torch.cuda.Stream:
    """a queue that is nobody else's (tavsr_stream_create): ``torch.cuda.Stream()`` comes out of a round-robin pool of 32 per device, and a
    side stream that later re-appears as some capture's stream would make the fork registry (keyed by raw handles) order that capture
    behind a stream outside it."""
    h = C.c_void_p(0)
    with torch.cuda.device(device):
        check(lib().tavsr_stream_create(C.byref(h)), "tavsr_stream_create")
    return torch.cuda.ExternalStream(h.value, device=device)


# Race amplifier (tests only): TAVSR_RACE_PROBE=<microseconds> enqueues a spin kernel at the head of every forked body
# ("body": the forked stream falls behind its owner - a main-pool block freed too early is overwritten under its readers),
# right after every join on the owning stream ("join": the owner falls behind - a forked-pool block handed out again too early
# is overwritten under the owner's readers), or alternately per scope ("alt", the default).  TAVSR_RACE_PROBE_MODE picks.
RACE_PROBE_US = float(os.environ.get("TAVSR_RACE_PROBE", "0") or 0)
RACE_PROBE_MODE = os.environ.get("TAVSR_RACE_PROBE_MODE", "alt")
_PROBE_TICK = [0]


def spin(us: float) -> None:
    """occupies the current stream for ``us`` microseconds (one wave polling the wall clock)"""
    check(lib().tavsr_spin(us, stream()), "tavsr_spin")


def arm_race_probe(us: float, mode: str = "alt") -> None:
    """(tests) set the amplifier at run time, for the Python-side scopes and the C-side sequencers alike"""
    global RACE_PROBE_US, RACE_PROBE_MODE
    RACE_PROBE_US, RACE_PROBE_MODE = float(us), mode
    check(lib().tavsr_race_probe(us, {"body": 0, "join": 1, "alt": 2}[mode]), "tavsr_race_probe")


def _probe(where: str, tick: int) -> None:
    if RACE_PROBE_US <= 0:
        return
    mode = RACE_PROBE_MODE
    if mode == "alt":
        mode = "body" if tick % 2 == 0 else "join"
    if mode == where:
        spin(RACE_PROBE_US)


class BranchScope:
    """``with BranchScope() as br: <launches>`` enqueues the body on the side stream (ordered after everything
    already on the main stream); ``br.join()`` orders the main stream after the body.
    Allocator safety (the two rules of _lib.py): tensors of the main stream's pool that the body hands to a launch are
    ``record_stream``-ed on the side stream as their pointers are taken (``_lib.ptr`` / ``_lib.addr``) - the main stream can
    free them whenever it likes; tensors allocated in the body live in the side stream's pool and are only handed out again
    to a later body, which starts with a wait on the main stream, so main-stream readers enqueued before that are always
    finished.  Capturable (fork/join inside one hipGraph capture)."""

    def __init__(self, enabled=True, slot=0):
        self.enabled = enabled and forks_enabled()
        self.slot = slot              # which of the owner's side streams (two scopes open at once take different slots)
        self.on = False               # (join() of a scope that was never entered is a no-op)

    def __enter__(self):
        self.main = torch.cuda.current_stream()
        self.on = self.enabled
        if self.on:
            self.side = branch_stream(self.main, self.slot)
            self.side.wait_stream(self.main)
            self.ctx = torch.cuda.stream(self.side)
            self.ctx.__enter__()
            self._prev = L.push_fork(self.side)
            self._tick = _PROBE_TICK[0]
            _PROBE_TICK[0] += 1
            _probe("body", self._tick)
        return self

    def __exit__(self, *exc):
        if self.on:
            L.pop_fork(self._prev)
            self.ctx.__exit__(*exc)
        return False

    def join(self):
        if self.on:
            self.main.wait_stream(self.side)
            _probe("join", self._tick)


# Weight gradients beside the backward chain.  A layer's weight gradients (one grouped launch of ~180 us at 12.4 rows per compute unit, the
# (dgamma, dbeta) partial sums behind it) have no consumer inside the backward pass; on the chain's own queue they sit between two layers
# whose first 150 us are one streaming FFN launch and eight latency-bound ones.  ``wgrad_beside(fn)`` enqueues them on the owner's side queue
# instead and does NOT join: the side queue is in-order, so the next layer's forked branch (and its join) comes behind them, and the end of the
# autograd pass joins what is still open (``Variable._execution_engine.queue_callback``).  Only taken when nobody reads the gradients before
# that: every parameter's ``.grad`` is None (AccumulateGrad then keeps the tensor, it does not add into one) and carries no hook other than
# this package's own bucket hooks, which fence themselves (``wgrad_fence``).
_WGRAD_OPEN = {}        # raw handle of the owning stream -> (owner, side) with weight-gradient launches nobody has joined yet


def wgrad_fence() -> None:
    """orders the CURRENT stream behind every weight-gradient launch that ``wgrad_beside`` left open (a no-op when there is none)"""
    if not _WGRAD_OPEN:
        return
    cur = torch.cuda.current_stream()
    capturing = torch.cuda.is_current_stream_capturing()
    for owner, side in list(_WGRAD_OPEN.values()):
        if capturing:
            with torch.cuda.stream(side):
                if not torch.cuda.is_current_stream_capturing():
                    continue       # left open by a pass that died before this capture began: not this graph's work (a capture cannot wait for it)
        cur.wait_stream(side)      # (only the calling stream: an owner that is itself a forked stream has been joined already - a wait enqueued
    _WGRAD_OPEN.clear()            # on it now would be work no capture ever joins)


def _wgrad_end_of_pass() -> None:
    wgrad_fence()


def _wgrad_callback() -> bool:
    """queues the end-of-pass join with the autograd pass that is running.  One per caller, not one per pass behind a flag: a pass that dies
    half-way (an out-of-memory error the training loop survives) never runs its callbacks, and a flag it had set would leave every later pass
    un-joined; a second ... twelfth callback of one pass finds nothing open and returns."""
    from torch.autograd import Variable
    try:
        Variable._execution_engine.queue_callback(_wgrad_end_of_pass)
    except RuntimeError:              # not inside an autograd pass (a test driving a backward by hand): nothing would join it
        return False
    return True


def wgrad_may_go_beside(params) -> bool:
    # (not in an instrumented pass: ``PROFILE`` brackets every GEMM launch with events to time the KERNEL - beside the chain a launch shares the
    # chip with whatever runs there, and bench.py's roofline would read 0.47 of peak for a kernel that does 0.63 alone)
    if not (ops.WGRAD_BESIDE and forks_enabled()) or ops.PROFILE is not None:
        return False
    for p_ in params:
        if p_ is None:
            continue
        if p_.grad is not None or p_._backward_hooks:
            return False
        if getattr(p_, "_post_accumulate_grad_hooks", None) and not getattr(p_, "_tavsr_hooks_fence", False):
            return False
    return True


def wgrad_open(main, side) -> bool:
    """(the C-side sequencer enqueues its weight gradients on ``side`` itself) notes them as open; False: not inside an autograd pass"""
    if not _wgrad_callback():
        return False
    _WGRAD_OPEN[main.cuda_stream] = (main, side)
    return True


def wgrad_beside(fn) -> None:
    """``fn()`` (launches only) on the side queue of the current stream, left open until the next ``wgrad_fence`` / the end of the pass"""
    if not _wgrad_callback():
        return fn()
    sc = BranchScope(True, slot=ops.WGRAD_SLOT)
    with sc:
        fn()
    if sc.on:
        _WGRAD_OPEN[sc.main.cuda_stream] = (sc.main, sc.side)


_BR_EVENTS = {}


def branch_events(main: torch.cuda.Stream):
    """(fork, join) events of the side stream that belongs to ``main`` (created once; recorded once so that the handles exist)."""
    key = (main.device.index, main.cuda_stream)
    ev = _BR_EVENTS.get(key)
    if ev is None:
        ev = (torch.cuda.Event(), torch.cuda.Event())
        for e in ev:
            e.record(main)
        _BR_EVENTS[key] = ev
    return ev
