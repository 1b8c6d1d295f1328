"""CPU (-m "not gpu"): the row-wise checker of tests/rowwise.py bites, and its yardstick is sound.

bf16(float32 emulation) stands in for the device, the float64 emulation (same bf16 operand roundings, everything else
double; each evaluation takes its own rounding decisions) is the reference.  Defects confined to a few rows are planted
in the stand-in: the whole-tensor relative L2 norm the GPU tests gate (EMU_TOL of tests/test_gpu_chain.py: 1e-2 for the
output and the rows gradient) is evaluated next to the row-wise check, which must fail on exactly the planted rows.
Rows are planted where the row norm is at least the rms row norm: the statistic is floored there on purpose, a 25 %
error of a near-zero row is small by design.

Soundness of the yardstick: a third honest evaluation (float32 with the views of every point reversed: other summation
orders in the BatchNorm, softmax and pooling sums) stays inside FP32_HEADROOM x the noise on every stratum."""
import pytest
import torch

import rowwise as RW
from oracle import pooling_oracle as O
from tolerances import FP32_HEADROOM, Report

OLD_GATE = 1e-2         # EMU_TOL["out"] == EMU_TOL["rows"] of tests/test_gpu_chain.py
R = 777


def ragged(N, gen):
    return torch.randint(0, 9, (N,), generator=gen)


def ragged_long(N, gen):
    s = torch.randint(0, 7, (N,), generator=gen)
    s[5], s[6], s[7], s[N - 1] = 100, 33, 64, 70
    return s


CASES = {"ragged_train": (ragged, 3000, 64, 4, True, True), "ragged_long_eval": (ragged_long, 2000, 64, 4, False, False),
         "ragged_long_c32": (ragged_long, 1500, 32, 2, True, True), "edges_c64": (RW.edges, 4001, 64, 4, True, True)}
_cache = {}


def rel(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).norm() / (b.norm() + 1e-12))


def case(name):
    """The inputs of test_chain_matches_bf16_emulation (same generator sequence) with the three evaluations."""
    if name in _cache:
        return _cache[name]
    sizes_fn, N, C, G, train, scaling = CASES[name]
    gen = torch.Generator().manual_seed(13)
    sizes = sizes_fn(N, gen)
    csr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    V = int(csr[-1])
    x_map = torch.rand(V, 8, generator=gen)
    w = torch.randn(N, C, generator=gen)
    rows = torch.randn(R, C, generator=gen).bfloat16()
    row_idx = torch.randint(0, R, (V,), generator=gen, dtype=torch.int32)
    ref = O.GroupBimodalCSRPool(in_map=8, in_mod=C, num_groups=G, use_num=True, gating=True, group_scaling=scaling)
    pg = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            p.copy_(torch.randn(p.shape, generator=pg) * 0.3)
            if "batch_norm.weight" in n or n == "G.weight":
                p.add_(1.0)
        for n, b in ref.named_buffers():
            if "running_mean" in n:
                b.copy_(torch.randn(b.shape, generator=pg) * 0.1)
            if "running_var" in n:
                b.copy_(torch.rand(b.shape, generator=pg) + 0.5)
    ref.train(train)
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    c = dict(name=name, N=N, C=C, G=G, V=V, csr=csr, x_map=x_map, w=w, rows=rows, row_idx=row_idx, ref=ref, sd=sd)
    c["e32"] = RW.emulate(ref, sd, rows, row_idx, x_map, csr, w)
    c["e64"] = RW.emulate(ref, sd, rows, row_idx, x_map, csr, w, dtype=torch.float64)
    c["seen"] = sizes > 0
    c["strata"] = RW.strata(csr)
    c["read"], c["read_live"] = RW.read_strata(row_idx, R)
    # the stand-in for the device: the float32 emulation rounded as the kernel rounds (bf16 output, bf16 rows gradient)
    c["dev_out"] = c["e32"]["out"].bfloat16()
    c["dev_rows"] = c["e32"]["rows_grad"].bfloat16()
    c["noise_out"] = RW.row_err(c["dev_out"], c["e64"]["out"], c["seen"])
    c["noise_rows"] = RW.row_err(c["dev_rows"], c["e64"]["rows_grad"], c["read_live"])
    _cache[name] = c
    return c


def check_out(c, dev_out, tag):
    rep = Report(f"row-wise host check: {c['name']} {tag}")
    err = RW.row_err(dev_out, c["e64"]["out"], c["seen"])
    RW.gate_rows(rep, c["name"], "out", err, c["noise_out"], c["strata"], c["seen"])
    return rep, err


def check_rows(c, dev_rows, tag):
    rep = Report(f"row-wise host check: {c['name']} {tag}")
    err = RW.row_err(dev_rows, c["e64"]["rows_grad"], c["read_live"])
    RW.gate_rows(rep, c["name"], "rows_grad", err, c["noise_rows"], c["read"], c["read_live"])
    return rep, err


def typical_row(ref_rows, live, skip=()):
    """The live row whose norm is the smallest one at or above the rms row norm (the floor of the statistic)."""
    nr = ref_rows.double().norm(dim=1)
    floor = nr[live].pow(2).mean().sqrt()
    cand = torch.where(live & (nr >= floor), nr, torch.full_like(nr, float("inf")))
    for s in skip:
        cand[s] = float("inf")
    i = int(cand.argmin())
    assert torch.isfinite(cand[i])
    return i


def fails_exactly(rep, err, noise, live, planted, masks):
    with pytest.raises(AssertionError):
        rep.check()
    bad = RW.failing_rows(err, noise, live).tolist()
    assert sorted(bad) == sorted(planted), (bad, planted)
    # every failed report row is a stratum that holds a planted row, and every stratum that holds one fails
    failed = set()
    for _, name, _, e, g, _ in rep.rows:
        if not e <= g:
            assert name.endswith("max"), name       # one or two rows of >= 200 do not move a p99
            failed.add(name[name.index("[") + 1:name.index(":")])
    holds = {"all"} | {k for k, m in masks.items() if any(bool(m[i]) for i in planted)}
    assert failed == holds, (failed, holds)


@pytest.mark.parametrize("name", ["ragged_train", "ragged_long_eval"])
def test_unplanted_stand_in_passes(name):
    c = case(name)
    rep, _ = check_out(c, c["dev_out"], "unplanted")
    rep.check()
    rep, _ = check_rows(c, c["dev_rows"], "unplanted")
    rep.check()
    unseen = ~c["seen"]
    assert float(c["e64"]["out"][unseen].abs().max()) == 0.0
    assert float(c["e64"]["rows_grad"][~c["read_live"]].abs().max() if (~c["read_live"]).any() else 0.0) == 0.0


@pytest.mark.parametrize("name", ["ragged_train", "ragged_long_eval"])
def test_a_one_point_scaled_passes_the_norm_and_fails_row_wise(name):
    c = case(name)
    i = typical_row(c["e64"]["out"], c["seen"])
    dev = c["dev_out"].clone()
    dev[i] = (dev[i].float() * 1.25).bfloat16()
    old = rel(dev, c["e32"]["out"])
    print(f"{name}: point {i} x 1.25: whole-tensor rel L2 {old:.2e} (gate {OLD_GATE:.0e})")
    assert old < OLD_GATE, "the claim: the whole-tensor norm lets this defect through"
    rep, err = check_out(c, dev, "one point x 1.25")
    fails_exactly(rep, err, c["noise_out"], c["seen"], [i], c["strata"])


@pytest.mark.parametrize("name", ["ragged_train", "ragged_long_eval"])
def test_b_neighbours_row_fails_row_wise(name):
    c = case(name)
    seen = c["seen"]
    i = typical_row(c["e64"]["out"], seen & torch.roll(seen, 1) & (torch.arange(c["N"]) > 0))
    dev = c["dev_out"].clone()
    dev[i] = dev[i - 1]
    old = rel(dev, c["e32"]["out"])
    print(f"{name}: point {i} receives the row of {i - 1}: whole-tensor rel L2 {old:.2e} "
          f"({'passes' if old < OLD_GATE else 'fails'} the gate {OLD_GATE:.0e})")
    rep, err = check_out(c, dev, "neighbour's row")
    fails_exactly(rep, err, c["noise_out"], seen, [i], c["strata"])


def test_c_dropped_fragment_tile_fails_row_wise():
    """The last point of ragged_long has 70 views = fragment tiles of 32 + 32 + 6: pooled over its first 64 only."""
    c = case("ragged_long_eval")
    csr, N, V = c["csr"], c["N"], c["V"]
    i = N - 1
    assert int(csr[i + 1] - csr[i]) == 70 and bool(c["strata"]["fragmented"][i])
    ref = c["ref"]
    ref.load_state_dict(c["sd"])
    keep = torch.ones(V, dtype=torch.bool)
    keep[int(csr[i]) + 64:int(csr[i + 1])] = False
    csr_cut = csr.clone()
    csr_cut[i + 1] = csr[i] + 64
    vals = c["rows"].float()[c["row_idx"].long()]
    with torch.no_grad():
        cut, _, _ = O.attention_tail(vals[keep], c["e32"]["scores"][keep], csr_cut, ref.G, ref.num_groups, ref.out_mod,
                                     ref.group_scaling)
    dev = c["dev_out"].clone()
    dev[i] = cut[i].bfloat16()
    old = rel(dev, c["e32"]["out"])
    print(f"70-view point pooled over 64 views: whole-tensor rel L2 {old:.2e} "
          f"({'passes' if old < OLD_GATE else 'fails'} the gate {OLD_GATE:.0e})")
    rep, err = check_out(c, dev, "dropped fragment tile")
    with pytest.raises(AssertionError):
        rep.check()
    assert RW.failing_rows(err, c["noise_out"], c["seen"]).tolist() == [i]
    failed = [n for _, n, _, e, g, _ in rep.rows if not e <= g]
    assert any("fragmented" in n for n in failed) and any("cloud_last" in n for n in failed), failed


@pytest.mark.parametrize("name", ["ragged_train", "ragged_long_eval"])
def test_d_last_seen_point_zeroed_fails_row_wise(name):
    c = case(name)
    i = int(torch.nonzero(c["seen"]).flatten()[-1])
    dev = c["dev_out"].clone()
    dev[i] = 0
    old = rel(dev, c["e32"]["out"])
    print(f"{name}: last seen point {i} zeroed: whole-tensor rel L2 {old:.2e} "
          f"({'passes' if old < OLD_GATE else 'fails'} the gate {OLD_GATE:.0e})")
    rep, err = check_out(c, dev, "last seen point zeroed")
    nr = c["e64"]["out"].norm(dim=1)
    if float(nr[i]) == 0.0:       # the gate of this point is exactly 0 (eval cases): zeroing it is no defect
        rep.check()
        return
    with pytest.raises(AssertionError):
        rep.check()
    assert RW.failing_rows(err, c["noise_out"], c["seen"]).tolist() == [i]
    assert any("cloud_last" in n for _, n, _, e, g, _ in rep.rows if not e <= g)


@pytest.mark.parametrize("name", ["ragged_train", "ragged_long_eval"])
def test_e_one_map_row_gradient_doubled_fails_row_wise(name):
    c = case(name)
    i = typical_row(c["e64"]["rows_grad"], c["read_live"])
    dev = c["dev_rows"].clone()
    dev[i] = (dev[i].float() * 2).bfloat16()
    old = rel(dev, c["e32"]["rows_grad"])
    print(f"{name}: map row {i} gradient doubled: whole-tensor rel L2 {old:.2e} "
          f"({'passes' if old < OLD_GATE else 'fails'} the gate {OLD_GATE:.0e})")
    rep, err = check_rows(c, dev, "one map row doubled")
    fails_exactly(rep, err, c["noise_rows"], c["read_live"], [i], c["read"])


@pytest.mark.parametrize("name", list(CASES))
def test_reversed_views_evaluation_stays_inside_the_gate(name):
    """The yardstick is sound: another honest float32 evaluation of the same case passes every stratum gate."""
    c = case(name)
    csr, V = c["csr"], c["V"]
    sizes = csr[1:] - csr[:-1]
    pid = torch.arange(c["N"]).repeat_interleave(sizes)
    perm = (csr[:-1][pid] + csr[1:][pid] - 1 - torch.arange(V))         # view v of a point <-> its mirror in the point
    assert torch.equal(torch.sort(perm).values, torch.arange(V))
    rev = RW.emulate(c["ref"], c["sd"], c["rows"], c["row_idx"][perm], c["x_map"][perm], csr, c["w"])
    rep = Report(f"reversed views against the float64 emulation: {name}")
    err = RW.row_err(rev["out"].bfloat16(), c["e64"]["out"], c["seen"])
    w1 = RW.gate_rows(rep, name, "out", err, c["noise_out"], c["strata"], c["seen"])
    err_r = RW.row_err(rev["rows_grad"].bfloat16(), c["e64"]["rows_grad"], c["read_live"])
    w2 = RW.gate_rows(rep, name, "rows_grad", err_r, c["noise_rows"], c["read"], c["read_live"])
    sc_noise = RW.score_err(c["e32"]["scores"], c["e64"]["scores"], csr)
    sc_err = RW.score_err(rev["scores"][perm], c["e64"]["scores"], csr)      # perm is an involution
    w3 = RW.gate_rows(rep, name, "scores", sc_err, sc_noise, c["strata"], c["seen"])
    print(f"{name}: worst ratio to the noise: out {w1:.2f} rows_grad {w2:.2f} scores {w3:.2f} (gate {FP32_HEADROOM})")
    rep.check()


def test_edges_sizes_fill_every_stratum():
    """The `edges` generator: every position class holds at least 16 points (host tile strata excepted: they need the
    device's table and are asserted by the GPU test), the total is a multiple of the chunk step."""
    c = case("edges_c64")
    sizes = c["csr"][1:] - c["csr"][:-1]
    assert c["V"] % RW.VIEWS_PER_CHUNK == 0 and RW.chunk_step(c["V"]) == RW.VIEWS_PER_CHUNK
    assert int(sizes[0]) == 0 and int(sizes[-1]) == 0
    for k in (0, 1, 2, 31, 32, 33, 63, 64, 65, 96, 100, 511, 512, 513, 5000):
        assert int((sizes == k).sum()) >= 3, k
    for name, m in c["strata"].items():
        if name.startswith("cloud_"):
            assert int(m.sum()) == 1
        else:
            assert int(m.sum()) >= 16, (name, int(m.sum()))


def test_strata_of_a_hand_made_table():
    """sizes 3, 0, 29, 32, 40, 1 -> tiles (0, 32, whole) (32, 32, whole) (64, 32, frag 1) (96, 8, frag 3) (104, 1, whole)."""
    csr = torch.tensor([0, 3, 3, 32, 64, 104, 105])
    tiles = torch.tensor([[0, 32], [32, 32], [64, 32 | (1 << 8)], [96, 8 | (3 << 8)], [104, 1]])
    s = RW.strata(csr, tiles, views_per_chunk=64)
    assert s["tile_first"].tolist() == [True, False, False, True, False, True]
    assert s["tile_last"].tolist() == [False, False, True, True, False, True]
    assert s["tile_interior"].tolist() == [False] * 6
    assert s["fragmented"].tolist() == [False, False, False, False, True, False]
    assert s["next_to_unseen"].tolist() == [True, False, True, False, False, False]
    assert s["cloud_first"].tolist() == [True] + [False] * 5 and s["cloud_last"].tolist() == [False] * 5 + [True]
    assert s["views_32"].tolist() == [False, False, False, True, False, False]
    # multiples of 64 (V = 105: two chunks of step 53 as well): 64 is the end of point 3 and the start of point 4
    assert s["chunk_edge"][3] and s["chunk_edge"][4] and not s["chunk_edge"][0]
    err = RW.row_err(torch.tensor([[3.0, 4.0], [0.0, 0.0], [0.0, 0.1]]), torch.tensor([[3.0, 0.0], [0.0, 0.0], [0.0, 0.0]]),
                     torch.tensor([True, False, True]))
    floor = (9.0 / 2) ** 0.5
    assert abs(float(err[0]) - 4.0 / 3.0) < 1e-12 and torch.isnan(err[1]) and abs(float(err[2]) - 0.1 / floor) < 1e-7


def test_open_finding_must_still_miss_its_gate_and_must_not_grow():
    """``gate_rows(open_findings=...)``: a recorded finding passes while it misses its gate at no more than 1.5 x the
    recorded value, fails once it has grown, and fails (as resolved) once the row meets its gate again."""
    c = case("ragged_train")
    i = typical_row(c["e64"]["out"], c["seen"])
    dev = c["dev_out"].clone()
    dev[i] = (dev[i].float() * 1.25).bfloat16()
    err = RW.row_err(dev, c["e64"]["out"], c["seen"])
    hit = [k for k, m in c["strata"].items() if bool(m[i])] + ["all"]

    def run(err, measured):
        rep = Report("open finding")
        RW.gate_rows(rep, c["name"], "out", err, c["noise_out"], c["strata"], c["seen"],
                     open_findings={("out", k, "max"): (measured, "planted") for k in hit})
        rep.check()
    run(err, float(err[i]))
    with pytest.raises(AssertionError, match="grew past"):
        run(err, float(err[i]) / 2)
    with pytest.raises(AssertionError, match="resolved"):
        run(RW.row_err(c["dev_out"], c["e64"]["out"], c["seen"]), float(err[i]))
