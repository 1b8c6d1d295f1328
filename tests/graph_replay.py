"""Replay of a captured step against an eager twin (DESIGN.md "Graph replay").  A plain helper module like rowwise.py
(not a conftest): tests import it by name.

What an eager test cannot see: a step captured once in a ``torch.cuda.CUDAGraph`` (= hipGraph) and replayed on NEW
contents of the same buffers goes wrong without a fault when an accumulator is zeroed outside the captured region, when
a constant was computed on the host from device data at capture time, when a plan built during warm-up is remembered,
or when running statistics are not updated in place.  ``run_replay`` runs the protocol:

 1. dry run: one eager ``step()`` under ``torch.cuda.set_sync_debug_mode("error")``; a step that synchronises raises
    ``HostSync`` and is never handed to the capture;
 2. warm-up: three steps on a side stream (``wait_stream`` both ways);
 3. capture: every ``.grad`` set to None, then one ``step()`` in ``torch.cuda.graph``;
 4. replay: ``contents[0]`` twice in a row, then every further entry once; before every replay the saved ``state`` and
    then the contents are ``copy_``-ed into the static tensors, after it every static tensor, every ``.grad`` and
    every output is cloned;
 5. eager twin: fresh tensors and a fresh module from the same state, default stream, no capture, the same sequence;
 6. clean-up: the graph is deleted and the device synchronised; the sync-debug mode is restored.

Gate, per tensor and per replay, replay against twin.  Yardstick: the twin is run ``YARDSTICK_RUNS`` times on every
content set; ``spread`` = the largest pairwise max-abs difference / the tensor's max-abs, the maximum over the content
sets.  spread == 0: the replay must equal the twin bit for bit (NaN == NaN).  spread > 0 (the eager path is itself
order-noisy: fp32 atomics): max|replay - twin| / max|twin| <= ``tolerances.REPLAY_HEADROOM`` x spread.  No bound is
typed in.  The eager noise is not one-humped (DESIGN.md "Graph replay": single discrete decisions behind an fp32 atomic
sum give a tensor a SECOND value in a fraction p of the runs), and n runs miss such a value with probability (1 - p)^n:
five runs missed the 22 % one of the C = 64 case 3 times in 10.  Hence 20 runs per content set, and where a row still
misses, ``EXTRA_RUNS`` further twin runs on the content set of that replay before the row is judged -- more samples of
the same quantity, the factor and the rule stay.
"""
import itertools

import pytest
import torch

from tolerances import REPLAY, REPLAY_HEADROOM, Report

WARMUP_STEPS = 3
YARDSTICK_RUNS = 20
EXTRA_RUNS = 80         # further twin runs on the content set of a replay whose row misses after YARDSTICK_RUNS
INF = float("inf")


class HostSync(AssertionError):
    """The dry run of a step synchronised with the host: the step is not capturable (and was not captured)."""


# ---------------------------------------------------------------------------------------------------------------
# gate arithmetic (host: tests/test_graph_replay_host.py runs it on recorded tensors)
# ---------------------------------------------------------------------------------------------------------------

def _f64(t):
    return t.detach().to("cpu").to(torch.float64)


def difference(got, want):
    """max|got - want| / max|want| in float64 (the plain max-abs difference where ``want`` is all zero); ``inf`` for a
    tensor on one side only, another shape or dtype, or a NaN on one side only.  Elements that compare equal (both
    +inf, say) and NaNs on both sides differ by 0.  0.0 for two tensors means ``torch.equal`` up to NaN == NaN."""
    if got is None and want is None:
        return 0.0
    if got is None or want is None or got.shape != want.shape or got.dtype != want.dtype:
        return INF
    if want.numel() == 0:
        return 0.0
    if want.dtype == torch.bool or not (want.dtype.is_floating_point or want.dtype.is_complex):
        return 0.0 if torch.equal(got.cpu(), want.cpu()) else INF        # integers and flags: exact or not at all
    g, w = _f64(got), _f64(want)
    if not torch.equal(g.isnan(), w.isnan()):
        return INF
    same = (g == w) | g.isnan()
    d = torch.where(same, torch.zeros_like(g), (g - w).abs())
    if bool(d.isnan().any()):                                            # inf against something else
        return INF
    num = float(d.max())
    den = float(w[torch.isfinite(w)].abs().max()) if bool(torch.isfinite(w).any()) else 0.0
    return num if den == 0.0 else num / den


def spread(samples):
    """Run-to-run spread of one tensor over repeated eager runs: the largest pairwise ``difference``.  (For finite
    floating-point samples evaluated in one pass: the largest entry of max - min over the runs is the largest pairwise
    max-abs difference; it is divided by the smallest max-abs of a run, the divisor of the pair that ``difference``
    would rate highest.)"""
    first = samples[0]
    plain = (all(torch.is_tensor(t) for t in samples) and first.dtype.is_floating_point and first.numel() > 0
             and all(t.shape == first.shape and t.dtype == first.dtype for t in samples))
    if plain:
        stack = torch.stack([t.detach().to(torch.float64) for t in samples])
        nan = stack.isnan()
        if bool((nan != nan[0]).any()):
            return INF
        if not bool(stack.isinf().any()):
            stack = torch.where(nan, torch.zeros_like(stack), stack).reshape(len(samples), -1)
            num = float((stack.amax(0) - stack.amin(0)).max())
            den = float(stack.abs().amax(1).min())
            return num if den == 0.0 else num / den
    return max((difference(a, b) for a, b in itertools.combinations(samples, 2)), default=0.0)


def yardstick(runs_per_content):
    """name -> spread, the maximum over the content sets; ``runs_per_content``: per content set a list of records
    (name -> tensor or None) of repeated runs on identical contents."""
    out = {}
    for runs in runs_per_content:
        for name in runs[0]:
            out[name] = max(out.get(name, 0.0), spread([r[name] for r in runs]))
    return out


def gate_records(rep, case, replayed, eager, spreads):
    """One Report row per tensor and replay: ``difference(replay, twin)`` against REPLAY_HEADROOM x the tensor's eager
    spread (0 -> bitwise).  A name recorded on one side only is a missing tensor: ``inf``.  Returns the worst ratio
    ``difference / spread`` over the order-noisy rows (0.0 when there is none)."""
    assert len(replayed) == len(eager), (len(replayed), len(eager))
    worst = 0.0
    for i, (got, want) in enumerate(zip(replayed, eager)):
        for name in sorted(set(got) | set(want)):
            if name not in got or name not in want:
                rep.add(f"{case} replay {i}", name, REPLAY, INF, 0.0, REPLAY_HEADROOM)
                continue
            s = spreads.get(name, 0.0)
            err = difference(got[name], want[name])
            rep.add(f"{case} replay {i}", name, REPLAY, err, s, REPLAY_HEADROOM)
            if s > 0:
                worst = max(worst, err / s)
    return worst


# ---------------------------------------------------------------------------------------------------------------
# the protocol (device)
# ---------------------------------------------------------------------------------------------------------------

def _load(statics, *dicts):
    with torch.no_grad():
        for d in dicts:
            for k, v in (d or {}).items():
                statics[k].copy_(v.to(statics[k].device))


def _drop_grads(statics):
    for t in statics.values():
        t.grad = None


def _record(statics, outs):
    rec = {}
    for k, t in statics.items():
        rec[k] = t.detach().clone()
        if t.requires_grad:
            rec[k + ".grad"] = None if t.grad is None else t.grad.detach().clone()
    for k, t in (outs or {}).items():
        rec["out:" + k] = None if t is None else t.detach().clone()
    return rec


def sync_debug_is_live(device):
    """Does ``set_sync_debug_mode("error")`` intercept ``.item()`` on this build?  Call with the mode set."""
    probe = torch.zeros(1, device=device)
    try:
        probe.item()
    except RuntimeError:
        return True
    return False


def dry_run(step, device):
    """One eager step under the sync-debug mode "error": ``HostSync`` if it synchronises with the host."""
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        if not sync_debug_is_live(device):
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not intercept .item() on this build")
        try:
            step()
        except RuntimeError as e:
            if "synchroniz" in str(e).lower():
                raise HostSync(f"the step synchronises with the host and is not captured: {e}") from e
            raise
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    torch.cuda.synchronize()


class Result:
    def __init__(self, report, replayed, eager, spreads, worst):
        self.report, self.replayed, self.eager, self.spreads, self.worst = report, replayed, eager, spreads, worst


def run_replay(step, statics, contents, state=None, twin=None, initial=None, title="graph replay", check=True):
    """``step()``: forward and ``loss.backward()`` on the static tensors (it enters ``torch.autocast`` itself, so that the
    capture contains the casts); it may return a dict name -> output tensor.  ``statics``: name -> tensor, the inputs,
    parameters and buffers; every one is compared after every step, and so is its ``.grad`` where it requires one.
    ``contents``: list of dicts name -> new value.  ``state``: name -> value restored before EVERY step (parameters,
    ``running_*``, ``num_batches_tracked``); ``initial``: name -> value restored before the FIRST step only (an
    accumulator the steps add into).  ``twin``: ``(step, statics)`` built once more from scratch (fresh tensors, a
    fresh module).  Returns a ``Result``; with ``check`` the Report is printed and asserted."""
    assert twin is not None, "run_replay needs the eager twin: (step, statics) built once more from scratch"
    twin_step, twin_statics = twin
    assert set(twin_statics) == set(statics)
    device = next(iter(statics.values())).device
    sequence = [contents[0]] + list(contents)
    graph = None
    previous = torch.cuda.get_sync_debug_mode()
    try:
        # 1. dry run: the first call of the step in this harness, so a first-call host read is seen as well
        _load(statics, initial, state, contents[0])
        dry_run(step, device)
        # 2. warm-up on a side stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(WARMUP_STEPS):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        # 3. capture
        _drop_grads(statics)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = step()
        torch.cuda.synchronize()
        # 4. replay
        replayed = []
        _load(statics, initial)
        for c in sequence:
            _load(statics, state, c)
            graph.replay()
            torch.cuda.synchronize()
            replayed.append(_record(statics, outs))
        # 5. eager twin: the yardstick, then the same sequence
        runs = [[] for _ in contents]

        def measure(ci, n):
            for _ in range(n):
                _load(twin_statics, initial, state, contents[ci])
                _drop_grads(twin_statics)
                runs[ci].append(_record(twin_statics, twin_step()))
        for ci in range(len(contents)):
            measure(ci, YARDSTICK_RUNS)
        eager = []
        _load(twin_statics, initial)
        for c in sequence:
            _load(twin_statics, state, c)
            _drop_grads(twin_statics)
            eager.append(_record(twin_statics, twin_step()))
        torch.cuda.synchronize()
        spreads = yardstick(runs)
        # a row that misses: further twin runs on the content set of that replay (replay i ran contents[max(i - 1, 0)])
        trial = Report("trial")
        gate_records(trial, title, replayed, eager, spreads)
        again = sorted({max(int(r[0].rsplit(" ", 1)[1]) - 1, 0) for r in trial.rows if not r[3] <= r[4]})
        for ci in again:
            measure(ci, EXTRA_RUNS)
        if again:
            spreads = yardstick(runs)
        torch.cuda.synchronize()
    finally:
        # 6. clean-up
        del graph
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode(previous)
    rep = Report(f"{title}: replay against the eager twin, gate = {REPLAY_HEADROOM:g} x the twin's run-to-run spread "
                 f"(0 = bit for bit)")
    worst = gate_records(rep, title, replayed, eager, spreads)
    noisy = {k: v for k, v in spreads.items() if v > 0}
    rep.notes.append(f"{len(spreads) - len(noisy)} of {len(spreads)} tensors have eager spread 0 (held bit for bit)")
    if noisy:
        k = max(noisy, key=noisy.get)
        rep.notes.append(f"largest eager spread {noisy[k]:.2e} ({k}); worst replay difference / spread {worst:.2f}")
    rep.notes.append(f"twin runs per content set: {[len(r) for r in runs]}")
    if check:
        rep.check()
    return Result(rep, replayed, eager, spreads, worst)
