"""The fp32 accuracy gates of the pooling path, in one place (DESIGN.md §2 lists them).

Metric: ``err = max|got - ref64| / max|ref64|`` per tensor, against a float64 evaluation of the same case (the
reference's own ``<name>_f64.npz`` fixtures, or the oracle module run in ``.double()``).  A tensor that is zero in
exact arithmetic (the ``E_score.bias`` gradient: the softmax ignores a shift common to all views of a point) is
measured against the max-abs of a named sibling tensor instead of its own ~1e-16.

A gate may go above its class gate only up to 4 x the error of a plain fp32 evaluation of the same case (the fp32
fixture against its float64 twin, or the oracle module run in torch fp32): ``gate(cls, fp32_err)`` computes that
bound from the measured number; it is never typed in.

The module is plain Python (not a conftest): tests import it by name.
"""
# fp32 against float64, by tensor class
CLASS_GATES = {
    "out": 1e-5,            # outputs and last_C / last_A / last_G
    "grad_in": 3e-5,        # input gradients
    "grad_param": 5e-5,     # parameter gradients
    "bn_mean": 1e-5,        # BatchNorm batch mean, in units of the batch standard deviation
    "bn_var": 2e-5,         # BatchNorm batch variance, relative
}
FP32_HEADROOM = 4.0         # how far above a plain fp32 evaluation's own error a gate may be raised

# Row-wise gates of the bf16 pooling path (tests/rowwise.py): per stratum of rows, the max and -- for strata of at least
# P99_MIN_ROWS rows -- the 99th percentile of the per-row error against the float64 emulation.  These classes have NO
# typed-in gate: the gate is FP32_HEADROOM x the same statistic of bf16(float32 emulation) against the float64
# emulation over all live rows of the case, computed at test time (AUTOCAST_ROW_HEADROOM x the statistic of the oracle
# under CPU autocast in the tests whose yardstick is that oracle: the factor they already use for whole outputs).
ROW_MAX, ROW_P99 = "row_max", "row_p99"
CLASS_GATES[ROW_MAX] = CLASS_GATES[ROW_P99] = 0.0
P99_MIN_ROWS = 200
AUTOCAST_ROW_HEADROOM = 1.5

# A captured step replayed on new contents against its eager twin (tests/graph_replay.py): NO typed-in gate either.  The
# gate is REPLAY_HEADROOM x the twin's own run-to-run spread on identical contents, measured at test time; a tensor
# whose spread is exactly 0 is held bit for bit.  (Five runs under-estimate the tail of ordering noise, hence 4 x; the
# defects aimed at -- a stale constant, an accumulator that keeps growing -- move results by orders of magnitude more.)
REPLAY = "replay"
CLASS_GATES[REPLAY] = 0.0
REPLAY_HEADROOM = 4.0

# parameter gradients that are zero in exact arithmetic when the module has no gate (a bias common to all views of a
# point) -> the sibling whose max-abs is the scale.  Used when the float64 tensor is below 1e-9 of that sibling.
STRUCTURAL_ZERO_SIBLING = {
    "E_score.bias": "E_score.weight",
    "K.bias": "K.weight",
}

# fp32 chain (fused_chain_f32) against float64 on the small random cases of test_gpu_chain3.py
CHAIN3_SCORES = dict(rtol=1e-5, atol=1e-5)
CHAIN3_PARAM_GRAD = 2e-5                    # tighter than the class gate: what that file held before

# product modules against the reference's fp32 golden fixtures (test_gpu_pool_modules.py, the fixture cases of
# test_gpu_chain3.py): the fixtures carry the host BLAS's own fp32 rounding (1e-7 .. 4e-5 of float64, amplified where
# terms cancel), so these are elementwise rtol / atol gates against fp32 and are NOT tightened here: the same cases are
# held to float64 at the class gates above by test_gpu_fp32_vs_f64.py::test_fixture_vs_f64, which is where the
# accuracy of these paths is enforced
FIXTURE_OUT = dict(rtol=1e-4, atol=1e-5)
FIXTURE_LAST_C = dict(rtol=5e-4, atol=1e-5)
FIXTURE_GRAD_IN = dict(rtol=1e-3, atol=1e-5)
FIXTURE_GRAD_PARAM = dict(rtol=2e-3, atol=3e-4)
FIXTURE_RUNNING = dict(rtol=1e-4, atol=1e-6)
ORACLE_RUNNING = dict(rtol=1e-4, atol=1e-5)


def rel_err(got, ref, scale=None):
    """max|got - ref| / max|scale| (scale defaults to ref), computed in float64."""
    g = got.detach().double()
    r = ref.detach().double().to(g.device)
    s = r if scale is None else scale.detach().double()
    den = float(s.abs().max()) if s.numel() else 0.0
    num = float((g - r).abs().max()) if g.numel() else 0.0
    if den == 0.0:          # exactly zero in float64 (a parameter the loss does not reach): the max-abs itself
        return num
    return num / den


def gate(cls, fp32_err=None, headroom=FP32_HEADROOM):
    """The enforced gate of a tensor of class ``cls``: the class gate, raised to at most ``headroom`` (FP32_HEADROOM
    unless the test's yardstick states its own factor) x the error of a plain evaluation of the same case when that
    error is known."""
    g = CLASS_GATES[cls]
    if fp32_err is not None:
        g = max(g, headroom * float(fp32_err))
    return g


def bn_errors(mean, var, mean64, var64):
    """(mean error in units of the float64 standard deviation, relative variance error), worst channel."""
    mean64, var64 = mean64.double(), var64.double()
    sd = var64.clamp_min(1e-300).sqrt()
    em = float(((mean.double().to(mean64.device) - mean64).abs() / sd).max())
    ev = float(((var.double().to(var64.device) - var64).abs() / var64.clamp_min(1e-300)).max())
    return em, ev


class Report:
    """Collects (case, tensor, class, err, gate) rows; ``check()`` prints the table (-s) and asserts every row."""

    def __init__(self, title):
        self.title, self.rows, self.open, self.notes = title, [], [], []

    def add(self, case, name, cls, err, fp32_err=None, headroom=FP32_HEADROOM):
        g = gate(cls, fp32_err, headroom)
        self.rows.append((case, name, cls, float(err), g, fp32_err))
        return err

    def add_open(self, case, name, cls, err, fp32_err, measured, why):
        """A named open finding: the row must still miss its gate (when it meets it, the finding is resolved and the
        entry goes) and must not grow past 1.5 x the error it was recorded with."""
        self.open.append((case, name, float(err), gate(cls, fp32_err), measured, why))
        self.add(case, name, cls, err, fp32_err)

    def table(self):
        lines = [f"== {self.title}", f"{'case':34s} {'tensor':46s} {'class':10s} {'err':>9s} {'gate':>9s} {'fp32':>9s}"]
        opened = {(c, n) for c, n, *_ in self.open}
        for case, name, cls, err, g, e32 in self.rows:
            flag = "" if err <= g else ("  OPEN" if (case, name) in opened else "  FAIL")
            e32s = f"{e32:9.2e}" if e32 is not None else f"{'-':>9s}"
            lines.append(f"{case:34s} {name:46s} {cls:10s} {err:9.2e} {g:9.2e} {e32s}{flag}")
        lines += ["   note: " + n for n in self.notes]
        return "\n".join(lines)

    def check(self):
        print("\n" + self.table())
        opened = {(c, n) for c, n, *_ in self.open}
        bad = [(c, n, e, g) for c, n, _, e, g, _ in self.rows if not e <= g and (c, n) not in opened]
        assert not bad, bad
        for c, n, e, g, measured, why in self.open:
            # (an entry recorded close to its gate can flip to "resolved" when the gate, itself a measured noise
            #  statistic, moves a little: the entry says so and is then taken out)
            assert e > g, f"{c} {n}: {e:.2e} now meets its gate {g:.2e} -- the open finding is resolved ({why})"
            assert e <= 1.5 * measured, f"{c} {n}: {e:.2e} grew past the recorded {measured:.2e} ({why})"


def param_scale(name, grads):
    """The tensor whose max-abs normalises the error of parameter gradient ``name`` (``grads``: name -> float64)."""
    own = grads[name]
    for suffix, sib in STRUCTURAL_ZERO_SIBLING.items():
        if name == suffix or name.endswith("." + suffix):
            other = grads[name[: len(name) - len(suffix)] + sib]
            if float(own.abs().max()) < 1e-9 * float(other.abs().max()):
                return other
    return own
