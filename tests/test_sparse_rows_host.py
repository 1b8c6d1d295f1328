"""CPU (-m "not gpu"): the row-wise gates of the sparse convolution (tests/sparse_rows.py) bite, and their yardstick is
sound.

The 3-term split evaluated in float32 stands in for the device, its float64 evaluation is the yardstick, the gate is
FP32_HEADROOM x the noise of the plain float32 evaluation -- exactly what tests/test_gpu_sparseconv.py does with the
kernel's output.  Soundness: a second honest float32 evaluation (the three terms summed in the opposite order) passes
every stratum.  Bite: defects of the size a subtly wrong kernel makes are planted in the stand-in; the whole-tensor
metric the GPU tests used to rely on alone (``max|got - exact64| <= 2e-5 max|exact64|``) is evaluated next to the row
gates, which must fail in the strata that hold the planted rows."""
import re

import pytest
import torch

import sparse_rows as SR
from oracle import sparseconv_oracle as O
from tolerances import Report

OLD_GATE = 2e-5
ALL_STRATA = ("nbr_1", "nbr_2_8", "nbr_9_26", "nbr_27", "tile_edge", "last_tile", "wave_skips", "wave_no_skip")


def case():
    return SR.conv_case("host_strata_96_64", SR.strata_cloud(1, 1500), 96, 64, bias=True)


def failed(rep):
    """{stratum name} of the report rows that miss their gate."""
    return {re.search(r"\[(\w+): \d+\]", name).group(1) for _, name, _, e, g, _ in rep.rows if not e <= g}


def check(c, **tensors):
    rep = Report("sparse rows host check")
    SR.gate_case(rep, c, require=ALL_STRATA, require_t=ALL_STRATA, **tensors)
    return rep


def split_trunc(t):
    """The planted defect: ``lo`` truncated to bf16 (the low 16 bits dropped) instead of rounded to nearest."""
    hi = t.bfloat16().float()
    lo = ((t - hi).view(torch.int32) & -65536).view(torch.float32)
    return hi, lo


def three_terms(c, split_x, split_w):
    xh, xl = split_x(c["x"])
    Wh, Wl = split_w(c["W"])
    return (O.sparse_conv(xh, Wh, None, c["nbr"]) + O.sparse_conv(xl, Wh, None, c["nbr"])
            + O.sparse_conv(xh, Wl, None, c["nbr"]) + c["b"])


def test_honest_evaluations_pass_every_stratum():
    c = case()
    other = dict(out=O.sparse_conv_split(c["x"], c["W"], c["b"], c["nbr"], order="hl,lh,hh"),
                 gx=O.sparse_conv_split(c["g"], c["W"].transpose(1, 2), None, c["nbr_t"], order="hl,lh,hh"),
                 gW=O.sparse_conv_split_grad_w(c["x"].flip(1), c["g"], c["nbr"]).flip(1),
                 gb=c["g"].flip(0).sum(0))
    for tensors in (dict(out=c["out32"], gx=c["gx32"], gW=c["gW32"], gb=c["gb32"]), other):
        rep = check(c, **tensors)
        rep.check()
    assert not torch.equal(other["out"], c["out32"])            # it IS another evaluation
    for key, ex in (("out", "out"), ("gx", "gx"), ("gW", "gW")):
        assert SR.old_metric(other[key], c["exact"][ex]) <= OLD_GATE


def test_truncated_lo_passes_the_old_metric_and_fails_the_rows():
    c = case()
    assert torch.equal(three_terms(c, O.split_bf16, O.split_bf16), c["out32"])     # the harness restates the healthy one
    bad = three_terms(c, split_trunc, split_trunc)
    assert SR.old_metric(bad, c["exact"]["out"]) <= OLD_GATE
    rep = check(c, out=bad)
    assert {"all", "nbr_1", "nbr_27", "wave_skips", "wave_no_skip"} <= failed(rep)
    with pytest.raises(AssertionError):
        rep.check()
    # ... and the wider gate the GPU tests state beside it (noise of the float32 evaluation in the kernel's
    # accumulation order, the proof behind the device's open findings) still catches it -- but not on the lone voxels,
    # whose chain is 18 additions long: that is what the plain gate is kept for
    wide = Report("kernel order")
    SR.gate_kernel_order(wide, c, bad, c["gx32"])
    assert {"all", "nbr_2_8", "nbr_9_26", "nbr_27", "wave_skips", "wave_no_skip"} <= failed(wide)
    honest = Report("kernel order, honest")
    SR.gate_kernel_order(honest, c, c["out32o"], c["gx32o"])
    SR.gate_kernel_order(honest, c, c["out32"], c["gx32"])
    honest.check()


def test_lost_lo_hi_term_of_one_block_fails_its_strata():
    """``xl Wh`` lost for one offset, 16 input channels and one 64-row block (a wavefront that skipped an MFMA)."""
    c = case()
    nbr = c["nbr"]
    skipped = SR.skipped_offsets(nbr)
    first_surface = SR.structured_part().shape[0] // 64 + 1
    no_skip = next(i for i in range(first_surface, len(skipped) - 1) if skipped[i] == 0)
    assert skipped[4] == 24                                     # rows 256 .. 319: the line
    for b0, expect in ((256, "wave_skips"), (64 * no_skip, "wave_no_skip")):
        masks = SR.conv_strata(nbr)
        rows = torch.arange(b0, b0 + 64)
        assert bool(masks[expect][rows].all())
        k = int((nbr[:, rows] >= 0).sum(1).argmax())
        hit = rows[nbr[k, rows] >= 0]
        _, xl = O.split_bf16(c["x"])
        Wh, _ = O.split_bf16(c["W"])
        bad = c["out32"].clone()
        bad[hit] -= xl[nbr[k, hit].long(), 32:48] @ Wh[k, 32:48]
        f = failed(check(c, out=bad))
        assert expect in f and "all" in f and any(n.startswith("nbr_") for n in f)
        other = "wave_no_skip" if expect == "wave_skips" else "wave_skips"
        assert other not in f


def test_defect_confined_to_the_lone_voxels_fails_their_stratum():
    c = case()
    lone = SR.conv_strata(c["nbr"])["nbr_1"]
    assert int(lone.sum()) >= 70
    bad = c["out32"].clone()
    bad[lone] = three_terms(c, split_trunc, split_trunc)[lone]  # `lo` truncated on these rows only
    assert SR.old_metric(bad, c["exact"]["out"]) <= OLD_GATE
    f = failed(check(c, out=bad))
    assert "nbr_1" in f and "all" in f and not f & {"nbr_2_8", "nbr_9_26", "nbr_27"}


def test_weight_gradient_rows_are_gated_too():
    """One offset's weight gradient with ``lo`` of grad_out truncated; offsets without a pair must be exactly zero."""
    c = case()
    gh, gl = split_trunc(c["g"])
    xh, xl = O.split_bf16(c["x"])
    k = 5
    dst = torch.nonzero(c["nbr"][k] >= 0).flatten()
    src = c["nbr"][k][dst].long()
    bad = c["gW32"].clone()
    bad[k] = xh[src].t() @ gh[dst] + xl[src].t() @ gh[dst] + xh[src].t() @ gl[dst]
    assert SR.old_metric(bad, c["exact"]["gW"]) <= OLD_GATE
    assert "all" in failed(check(c, gW=bad))
    tiny = SR.conv_case("host_n1", SR.strata_cloud(1, 0)[:1], 32, 64)
    masks, live = SR.wgrad_strata(tiny["nbr"], 32, require=("pairs_1_31",))
    assert int(live.sum()) == 32
    dirty = tiny["gW32"].clone()
    dirty[0, 0, 0] = 1e-30
    with pytest.raises(AssertionError, match="dead row"):
        check_tiny = Report("dead rows")
        SR.gate_case(check_tiny, tiny, gW=dirty)
