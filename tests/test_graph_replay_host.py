"""The gate arithmetic of tests/graph_replay.py on recorded tensors (CPU), and -- marked gpu -- two planted stand-ins
that prove the harness bites: plain torch steps, no project kernel, each with the defect a captured step can have
without faulting and with its corrected form next to it (the planted / unplanted pattern of test_rowwise_host.py)."""
import pytest
import torch

import graph_replay as GR
from tolerances import REPLAY_HEADROOM, Report

DEV = "cuda:0"


def _gate(replayed, eager, spreads):
    rep = Report("host")
    worst = GR.gate_records(rep, "host", replayed, eager, spreads)
    return rep, worst


def _fails(rep):
    with pytest.raises(AssertionError):
        rep.check()


def test_zero_spread_demands_the_same_bits():
    gen = torch.Generator().manual_seed(0)
    a = torch.randn(50, 7, generator=gen)
    runs = [[{"x": a.clone()} for _ in range(5)]]
    spreads = GR.yardstick(runs)
    assert spreads == {"x": 0.0}
    rep, worst = _gate([{"x": a.clone()}], [{"x": a}], spreads)
    rep.check()
    assert worst == 0.0
    b = a.clone()
    b[3, 2] = torch.nextafter(b[3, 2], torch.tensor(10.0))            # one ulp in one element
    rep, _ = _gate([{"x": b}], [{"x": a}], spreads)
    _fails(rep)
    # integers: exact or not at all, whatever the spread says
    n = torch.arange(12).reshape(3, 4)
    m = n.clone()
    m[1, 1] += 1
    assert GR.difference(n.clone(), n) == 0.0 and GR.difference(m, n) == GR.INF
    rep, _ = _gate([{"n": m}], [{"n": n}], {"n": 0.0})
    _fails(rep)


def test_noisy_spread_allows_its_ratio_and_no_more():
    gen = torch.Generator().manual_seed(1)
    a = torch.randn(200, generator=gen, dtype=torch.float64)    # float64: a + e carries no rounding of its own
    a[17] = 4.0                                                        # the max-abs that normalises
    noise = [1e-6 * torch.randn(200, generator=gen, dtype=torch.float64) for _ in range(5)]
    for e in noise:
        e[17] = 0.0
    runs = [[{"g": a + e} for e in noise]]
    s = GR.yardstick(runs)["g"]
    want = max(float((x - y).abs().max()) for x in noise for y in noise) / 4.0
    assert s == pytest.approx(want, rel=1e-5) and s > 0
    # the one-pass form equals the pairwise definition
    assert s == pytest.approx(max(GR.difference(x["g"], y["g"]) for x in runs[0] for y in runs[0]), rel=1e-4)
    # a second value in one run of twenty (a two-valued eager tensor) is the spread as soon as it is sampled once
    jump = a.clone()
    jump[9] += 1e-3
    assert GR.spread([a.clone() for _ in range(19)] + [jump]) == pytest.approx(1e-3 / 4.0, rel=1e-9)
    # the maximum over the content sets
    assert GR.yardstick(runs + [[{"g": a.clone()} for _ in range(5)]])["g"] == s
    inside, outside = a.clone(), a.clone()
    inside[5] += 0.9 * REPLAY_HEADROOM * s * 4.0
    outside[5] += 1.2 * REPLAY_HEADROOM * s * 4.0
    rep, worst = _gate([{"g": inside}], [{"g": a}], {"g": s})
    rep.check()
    assert worst == pytest.approx(0.9 * REPLAY_HEADROOM, rel=1e-3)
    rep, worst = _gate([{"g": outside}], [{"g": a}], {"g": s})
    _fails(rep)
    # what the harness is for: a stale constant (x 1.01) or an accumulator that grew (x 2) is far outside
    for factor in (1.01, 2.0):
        rep, worst = _gate([{"g": a * factor}], [{"g": a}], {"g": s})
        _fails(rep)
        assert worst > 1e3


def test_nan_equals_nan_and_nothing_else():
    nan = torch.tensor(float("nan"))
    assert GR.difference(nan.clone(), nan) == 0.0                     # the loss when every label is ignored
    assert GR.difference(torch.tensor(0.0), nan) == GR.INF and GR.difference(nan, torch.tensor(0.0)) == GR.INF
    a = torch.tensor([1.0, float("nan"), float("inf"), -2.0])
    assert GR.difference(a.clone(), a) == 0.0
    assert GR.difference(torch.tensor([1.0, float("nan"), 3.0, -2.0]), a) == GR.INF        # inf against a number
    assert GR.difference(torch.tensor([1.0, 2.0, float("inf"), -2.0]), a) == GR.INF        # NaN on one side
    assert GR.spread([nan.clone() for _ in range(5)]) == 0.0
    rep, _ = _gate([{"loss": nan.clone()}], [{"loss": nan}], {"loss": 0.0})
    rep.check()
    rep, _ = _gate([{"loss": torch.tensor(0.5)}], [{"loss": nan}], {"loss": 0.0})
    _fails(rep)
    # an all-zero twin (the gradient of an all-zero map): the plain difference, no division
    z = torch.zeros(9)
    assert GR.difference(z.clone(), z) == 0.0 and GR.difference(z + 1e-30, z) == pytest.approx(1e-30)
    # another dtype or shape is no match
    assert GR.difference(z.double(), z) == GR.INF and GR.difference(z[:8], z) == GR.INF


def test_missing_gradient_fails():
    g = torch.ones(4)
    assert GR.difference(None, None) == 0.0                            # no gradient on either side: nothing to hold
    assert GR.difference(None, g) == GR.INF and GR.difference(g, None) == GR.INF
    rep, _ = _gate([{"w.grad": None}], [{"w.grad": None}], {"w.grad": 0.0})
    rep.check()
    rep, _ = _gate([{"w.grad": None}], [{"w.grad": g}], {"w.grad": 0.0})
    _fails(rep)
    rep, _ = _gate([{"w.grad": g}], [{"w.grad": None}], {"w.grad": 1e-3})
    _fails(rep)
    rep, _ = _gate([{}], [{"w.grad": g}], {"w.grad": 0.0})             # not recorded at all on one side
    _fails(rep)
    with pytest.raises(AssertionError):                                # a replay too few
        _gate([{"w.grad": g}], [{"w.grad": g}, {"w.grad": g}], {})


# ---------------------------------------------------------------------------------------------------------------
# planted stand-ins (gpu): plain torch, no project kernel
# ---------------------------------------------------------------------------------------------------------------

def _standin(kind, primed=False):
    """(step, statics) of y = (x @ w) * scale, loss = sum(y).

    'zero_outside' / 'zero_inside': scale = mean(acc) with acc = column sums of |x|, accumulated into a zero buffer.
    Planted, the buffer is the next piece of a pool that was zero-filled when the step was built (every eager call
    takes a piece nobody has written; a replay adds into the piece of the capture once more: right the first time,
    twice the sum the second time -- why contents[0] is replayed twice).  Corrected, the step fills its own zeros.

    'host_scale' / 'device_scale': scale = max|x|.  Planted, it is a Python float read from x on the first call and
    remembered, and that first call happened before the harness saw the step (``primed``: a warm-up somewhere else),
    so no synchronisation is left for the dry run to object to.  Corrected, it stays on the device."""
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(64, 16, generator=gen).to(DEV)
    w = torch.randn(16, 8, generator=gen).to(DEV).requires_grad_()
    statics = dict(x=x, w=w)
    pool, taken, memo = torch.zeros(64, 16, device=DEV), [0], {}

    def step():
        if kind in ("zero_outside", "zero_inside"):
            if kind == "zero_outside":
                acc = pool[taken[0]]
                taken[0] += 1
            else:
                acc = torch.zeros(16, device=DEV)
            acc.add_(x.abs().sum(0))
            scale = acc.mean()
        elif kind == "host_scale":
            if "scale" not in memo:
                memo["scale"] = float(x.abs().max())
            scale = memo["scale"]
        else:
            scale = x.abs().max()
        y = (x @ w) * scale
        y.sum().backward()
        return {"y": y}
    if primed:
        step()
        w.grad = None
    return step, statics


def _contents():
    gen = torch.Generator().manual_seed(5)
    return [dict(x=torch.randn(64, 16, generator=gen) * s) for s in (1.0, 3.0, 0.25)]


@pytest.mark.gpu
@pytest.mark.parametrize("planted,corrected", [("zero_outside", "zero_inside"), ("host_scale", "device_scale")])
def test_planted_standins_are_rejected_and_their_corrected_forms_pass(planted, corrected):
    step, statics = _standin(corrected)
    res = GR.run_replay(step, statics, _contents(), twin=_standin(corrected), title=f"stand-in {corrected}")
    assert len(res.replayed) == 4
    step, statics = _standin(planted, primed=True)
    res = GR.run_replay(step, statics, _contents(), twin=_standin(corrected), title=f"stand-in {planted}", check=False)
    with pytest.raises(AssertionError):
        res.report.check()
    bad = [r for r in res.report.rows if not r[3] <= r[4]]
    if planted == "host_scale":
        # not primed, the read from the data happens in the dry run, which is the first call: never captured
        step, statics = _standin(planted)
        with pytest.raises(GR.HostSync):
            GR.run_replay(step, statics, _contents(), twin=_standin(corrected), title="stand-in host_scale, first call")
    if planted == "zero_outside":
        # the first replay adds into a piece that is still zero: only the second replay of the same contents shows it
        assert not [r for r in bad if r[0].endswith("replay 0")] and [r for r in bad if r[0].endswith("replay 1")]
    # the defect moves the results by orders of magnitude more than any ordering noise would
    assert bad and max(r[3] for r in bad) > 1e-2, bad
