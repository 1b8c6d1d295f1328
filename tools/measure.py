"""What the side benchmarks (``tools/*_bench.py``) share: the timed windows, the loop that alternates the arms of a
comparison, the summary of a list of times, the counters of one call, and the head and tail of a record.

Clocks.  ``host_window`` is the host clock around ``inner`` calls between two device synchronisations, for anything
that ends on the host; ``event_window`` is two device events around ``inner`` calls, for work that stays on the device;
``both_window`` takes both from one window.  All return milliseconds per call.

Protocol.  ``alternate`` warms every arm up, drains the device, and then times the arms in turn inside every
repetition, so that drift of the machine falls on all arms alike.  With ``seconds`` a window holds as many calls as fill
that time, found from a short probe window.

Counters.  ``profile_once`` reports of one call: ``torch_ops``, the aten operator calls that take or return a device
tensor (each at least one kernel or copy); ``dva_launches``, the calls into the HIP library; ``syncs``, the host
synchronisations torch's sync debug mode warns of; ``peak_bytes``, the peak of allocated device memory above what was
resident before the call.  ``profiler_kernel_count`` is another quantity: the device kernels the torch profiler sees.

``alternate`` with an injected window, ``summarise``, ``ranges_overlap`` and ``emit`` need neither torch nor a device.
"""
import contextlib
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


# ---- windows ---------------------------------------------------------------------------------------------------

def event_window(fn, inner=1):
    """ms per call between two device events around ``inner`` calls."""
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / inner


def host_window(fn, inner=1):
    """ms per call on the host clock: synchronise, ``inner`` calls, synchronise."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def both_window(fn, inner=1):
    """(host ms, device ms) per call from one window: the events lie inside the two synchronisations."""
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(inner):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner, start.elapsed_time(stop) / inner


def _drain():
    """Wait for the warm-up calls, where a device is in use."""
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_initialized():
        torch.cuda.synchronize()


# ---- the loop --------------------------------------------------------------------------------------------------

def alternate(arms, reps, window, warmup=1, seconds=None, before=None, caps=None, probe_inner=1):
    """Time ``arms`` ({name: callable}) for ``reps`` repetitions, the arms in the order given inside every one.

    ``window(fn, inner)`` returns the ms of one timed window; ``window`` and ``warmup`` may be a dict by arm name where
    the arms differ.  Every arm is called ``warmup`` times before any timed window.  With ``seconds``, ``inner`` of an
    arm is ``max(1, int(seconds * 1e3 / probe_ms))`` from one probe window of ``probe_inner`` calls; without, 1.
    ``caps`` ({name: n}) ends an arm after n repetitions.  ``before(name, rep)`` runs outside the timed region before
    every call of an arm: ``rep`` is None in the warm-up and the probe, the repetition before a timed window.
    Returns ({name: [ms of every window]}, {name: inner})."""
    per_arm = lambda v: v if isinstance(v, dict) else dict.fromkeys(arms, v)
    window, warmup, caps = per_arm(window), per_arm(warmup), caps or {}
    before = before or (lambda name, rep: None)
    inner = dict.fromkeys(arms, 1)
    for name, fn in arms.items():
        for _ in range(warmup[name]):
            before(name, None)
            fn()
        if seconds is not None:
            _drain()
            before(name, None)
            inner[name] = max(1, int(seconds * 1e3 / max(window[name](fn, probe_inner), 1e-3)))
    _drain()
    ms = {name: [] for name in arms}
    for rep in range(reps):
        for name, fn in arms.items():
            if rep < caps.get(name, reps):
                before(name, rep)
                ms[name].append(window[name](fn, inner[name]))
    return ms, inner


def repeated(fn, reps, window, warmup=1):
    """The ms of ``reps`` windows of one call of ``fn`` after ``warmup`` untimed calls: ``alternate`` with one arm."""
    return alternate({"fn": fn}, reps, window, warmup=warmup)[0]["fn"]


# ---- summaries -------------------------------------------------------------------------------------------------

def summarise(ms, digits):
    """Median, min, max and spread (max - min) of ``ms``, rounded; the caller picks the names of its record."""
    if not ms:
        raise ValueError("summarise needs at least one measurement")
    return {"median": round(statistics.median(ms), digits), "min": round(min(ms), digits),
            "max": round(max(ms), digits), "spread": round(max(ms) - min(ms), digits)}


def ranges_overlap(a, b):
    """Whether the closed ranges a = (min, max) and b = (min, max) share a point."""
    return not (a[0] > b[1] or b[0] > a[1])


# ---- counters --------------------------------------------------------------------------------------------------

class CountLaunches:
    """ops.TIMER stand-in: records the calls into the HIP library, no events."""

    def __init__(self):
        self.names = []

    def launch(self, name, nbytes):
        from deepviewagg_amd import ops
        self.names.append(name)
        return ops._NO_TIMER


@contextlib.contextmanager
def launch_counter():
    """A CountLaunches as ops.TIMER inside the block; ops.TIMER is what it was afterwards."""
    from deepviewagg_amd import ops
    found, counter = ops.TIMER, CountLaunches()
    ops.TIMER = counter
    try:
        yield counter
    finally:
        ops.TIMER = found


def _count_device_ops():
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode

    class CountDeviceOps(TorchDispatchMode):
        """Counts the aten operator calls that take or return a device tensor."""

        def __init__(self):
            super().__init__()
            self.n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            flat = list(args) + list((kwargs or {}).values()) + (list(out) if isinstance(out, (tuple, list)) else [out])
            if any(torch.is_tensor(a) and a.is_cuda for a in flat):
                self.n += 1
            return out

    return CountDeviceOps()


@contextlib.contextmanager
def sync_warnings():
    """The warnings of torch's sync debug mode inside the block, as a list that is filled on leaving it.  A warning
    counts if it reports a synchronising operation; the mode's own notice that it is a prototype does not."""
    import torch
    counted = []
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            yield counted
    finally:
        torch.cuda.set_sync_debug_mode("default")
        counted += [w for w in seen if "synchroniz" in str(w.message).lower()
                    and "prototype" not in str(w.message).lower()]


@contextlib.contextmanager
def peak_memory():
    """The peak of allocated device memory inside the block above what was allocated on entering it, as a one-item
    list that is filled on leaving the block."""
    import torch
    peak = []
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    try:
        yield peak
    finally:
        torch.cuda.synchronize()
        peak.append(int(torch.cuda.max_memory_allocated() - base))


def peak_bytes(fn):
    with peak_memory() as peak:
        fn()
    return peak[0]


def profile_once(fn):
    """What one call of ``fn`` does: {torch_ops, dva_launches, syncs, peak_bytes} (see the module's docstring)."""
    with peak_memory() as peak, launch_counter() as launches, sync_warnings() as syncs, _count_device_ops() as mode:
        fn()
    return {"torch_ops": mode.n, "dva_launches": len(launches.names), "syncs": len(syncs), "peak_bytes": peak[0]}


def profiler_kernel_count(fn):
    """The device kernels of one call as the torch profiler counts them (after one untimed call); None where the
    profiler is not available.  Not the same quantity as ``dva_launches``."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return int(sum(e.count for e in prof.key_averages()
                       if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()))
    except Exception as exc:        # no tracer on this install: not measured
        print(f"kernel count not measured: {exc!r}", file=sys.stderr)
        return None


# ---- records ---------------------------------------------------------------------------------------------------

def header(tool, **fields):
    """The head of a record: the tool, the device and the build it measured, then the tool's own fields."""
    import torch
    from deepviewagg_amd import _lib
    return {"tool": tool, "device": torch.cuda.get_device_name(0), "dva_version": _lib.load().dva_version(),
            "source_sha256": _lib.source_sha256(), **fields}


def emit(result, out=None):
    """One JSON line on stdout, and in ``out`` where given (its directory is made)."""
    line = json.dumps(result)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
