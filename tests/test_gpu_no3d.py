"""GPU: the tail of the image-only models -- ``ops.nearest_seen`` / ``ops.fill_unseen`` (csrc/nearest_seen.hip),
``ops.view_nll`` (csrc/view_loss.hip), ``models.no3d.no3d_tail`` and ``UnimodalBranch.KEEP_LAST_VIEW_LAZY`` -- against the
CPU restatements of tests/no3d_ref.py.

nearest seen: ``src`` bit for bit the float32 brute force (lowest index on ties) on every cloud; on the uniform clouds
also the float64 brute force on every query outside the margin whose size tests/test_no3d_host.py caps.
view loss: float64 evaluation of the materialised formula at the class gates of tests/tolerances.py, each passed through
``gate(cls, fp32_err)`` with the error of the plain float32 torch composition on the same case."""
import functools

import pytest
import torch
import torch.nn.functional as F

import no3d_ref as R
import tolerances as T
from deepviewagg_amd import ops
from deepviewagg_amd.models import no3d

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CLOUDS = {name: (pos, seen) for name, pos, seen in list(R.uniform_cases()) + list(R.special_cases())}


@functools.lru_cache(maxsize=None)
def src_ref(name):
    """float32 brute force of a cloud, computed once and shared."""
    pos, seen = CLOUDS[name]
    return R.nearest_seen_ref(pos, seen)


def on_device(name):
    pos, seen = CLOUDS[name]
    return pos.to(DEV), seen.to(DEV)


# ---------------------------------------------------------------------------------------------
# nearest_seen / fill_unseen
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CLOUDS))
def test_nearest_seen_is_the_brute_force(name):
    pos, seen = on_device(name)
    want = src_ref(name)
    src, any_seen = ops.nearest_seen(pos, seen)
    assert src.dtype == torch.int32 and any_seen.dtype == torch.bool and any_seen.shape == (1,)
    assert torch.equal(src.cpu().long(), want), name
    assert bool(any_seen) == bool(CLOUDS[name][1].any())
    again, _ = ops.nearest_seen(pos, seen)
    assert torch.equal(src, again)
    # uint8 mask, and the composition this op replaces: compact, query, map back
    src8, _ = ops.nearest_seen(pos, seen.to(torch.uint8))
    assert torch.equal(src8, src)
    if bool(seen.any()) and not bool(seen.all()):
        nbr, _ = ops.knn_query(pos[~seen], pos[seen], 1)
        comp = torch.arange(pos.shape[0], device=DEV)
        comp[~seen] = torch.nonzero(seen).flatten()[nbr[:, 0].long()]
        assert torch.equal(comp, src.long())


# (clouds without a query or without a candidate leave a float64 search nothing to decide differently)
@pytest.mark.parametrize("name", [n for n, (_, m) in CLOUDS.items()
                                  if n.startswith("uniform") and bool(m.any()) and not bool(m.all())])
def test_nearest_seen_against_float64_outside_the_margin(name):
    pos_c, seen_c = CLOUDS[name]
    pos, seen = on_device(name)
    src, _ = ops.nearest_seen(pos, seen)
    want, d1, d2 = R.nearest_seen_ref(pos_c, seen_c, torch.float64, with_margin=True)
    held = ~R.in_margin(d1, d2)
    assert torch.equal(src.cpu().long()[held], want[held])


@pytest.mark.parametrize("cell", [0.013, 0.4, 9.0, 5000.0])
@pytest.mark.parametrize("name", ["uniform3000-f0.3", "uniform4097-corner", "clusters-one-side", "voxel14-f0.02",
                                  "planar-f0.3", "uniform65-one"])
def test_nearest_seen_is_exact_for_any_cell(name, cell):
    pos, seen = on_device(name)
    src, _ = ops.nearest_seen(pos, seen, cell=cell)
    assert torch.equal(src.cpu().long(), src_ref(name))


def payload(n, K, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, K, generator=gen)
    flat = x.view(-1)
    flat[0::7] = float("nan")
    flat[3::11] = float("inf")
    flat[5::13] = float("-inf")
    return x.to(dtype)


def same_bits(a, b):
    view = torch.int32 if a.element_size() == 4 else torch.int16
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(view), b.view(view))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K", [1, 13, 20, 64])
@pytest.mark.parametrize("name", ["uniform4097-f0.3", "uniform65-f0.5", "uniform63-none", "uniform64-all", "uniform1-none",
                                  "duplicates-f0.5"])
def test_fill_unseen_copies_rows_as_bits(name, K, dtype):
    pos, seen = on_device(name)
    n = pos.shape[0]
    x = payload(n, K, dtype, seed=K).to(DEV)
    keep = x.clone()
    filled, any_seen = ops.fill_unseen(x, pos, seen)
    assert same_bits(x, keep), "the input is left as it is"
    want = x[src_ref(name).to(DEV)]
    assert same_bits(filled, want)
    assert bool(any_seen) == bool(CLOUDS[name][1].any())
    if not bool(any_seen):
        assert same_bits(filled, x)
    again, _ = ops.fill_unseen(x, pos, seen)
    assert same_bits(filled, again)
    assert not filled.requires_grad


def test_fill_unseen_detaches_and_takes_an_empty_cloud():
    x = torch.randn(65, 13, device=DEV, requires_grad=True)
    pos, seen = on_device("uniform65-f0.5")
    filled, _ = ops.fill_unseen(x, pos, seen)
    assert not filled.requires_grad
    filled, any_seen = ops.fill_unseen(torch.zeros(0, 13, device=DEV), torch.zeros(0, 3, device=DEV),
                                       torch.zeros(0, dtype=torch.bool, device=DEV))
    assert filled.shape == (0, 13) and not bool(any_seen)
    src, _ = ops.nearest_seen(torch.zeros(0, 3, device=DEV), torch.zeros(0, dtype=torch.bool, device=DEV))
    assert src.shape == (0,)


def test_fill_unseen_with_a_cell_never_reads_the_host():
    pos, seen = on_device("uniform3000-f0.3")
    x = payload(3000, 20, torch.float32, seed=1).to(DEV)
    ops.fill_unseen(x, pos, seen, cell=0.2)                      # workspace sizes, library load: outside the section
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        filled, any_seen = ops.fill_unseen(x, pos, seen, cell=0.2)
        src, _ = ops.nearest_seen(pos, seen, cell=0.2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert same_bits(filled, x[src_ref("uniform3000-f0.3").to(DEV)])
    assert torch.equal(src.cpu().long(), src_ref("uniform3000-f0.3"))


# ---------------------------------------------------------------------------------------------
# view_nll
# ---------------------------------------------------------------------------------------------

def view_inputs(case, kind, dtype):
    """(x_view for ops.view_nll, leaf tensor that receives the gradient, materialise(leaf on the CPU) -> [V, K])."""
    rows = case["rows"].to(dtype).to(DEV).requires_grad_()
    row_idx = case["row_idx"].to(DEV)
    R_ = rows.shape[0]
    if kind == "lazy":
        counts = torch.bincount(row_idx.long(), minlength=R_).int()
        return ops.GatheredFeatures(rows, row_idx, counts, True), rows, lambda r: r[case["row_idx"].long()]
    if kind == "cat":          # two settings stacked, views permuted: what UnimodalBranch hands on for a multi-setting batch
        half = R_ // 2
        V = row_idx.shape[0]
        first = row_idx < half
        order = torch.cat([torch.nonzero(first).flatten(), torch.nonzero(~first).flatten()]).argsort()
        a = ops.GatheredFeatures(rows[:half], row_idx[first], torch.zeros(half, dtype=torch.int32, device=DEV), True)
        b = ops.GatheredFeatures(rows[half:], row_idx[~first] - half, torch.zeros(R_ - half, dtype=torch.int32, device=DEV),
                                 True)
        cat = ops.GatheredFeatures.cat([a, b], order=order)
        assert cat.row_idx.shape[0] == V
        return cat, rows, lambda r: r[case["row_idx"].long()]
    if kind == "identity":     # what an atomic gather_segment_reduce returns: the pooled [V, K] rows under the identity index
        xv = case["rows"][case["row_idx"].long()].to(dtype).to(DEV).requires_grad_()
        V = xv.shape[0]
        ident = torch.arange(V + 1, dtype=torch.int32, device=DEV)
        return (ops.GatheredFeatures(xv, ident[:V], torch.ones(V, dtype=torch.int32, device=DEV), True, (ident[:V], ident)),
                xv, lambda r: r)
    assert kind == "tensor"
    xv = case["rows"][case["row_idx"].long()].to(dtype).to(DEV).requires_grad_()
    return xv, xv, lambda r: r


def torch_view_loss(x_view, labels, csr_idx, weight, dtype):
    """The materialised composition in ``dtype`` on the CPU, with its gradient to x_view."""
    x = x_view.detach().cpu().to(dtype).requires_grad_()
    lab = labels.clone()
    lab[(lab < 0) | (lab >= x.shape[1])] = R.IGNORE_LABEL            # torch asserts on an out-of-range target
    target = lab.repeat_interleave(csr_idx[1:] - csr_idx[:-1])
    w = None if weight is None else weight.to(dtype)
    loss = F.nll_loss(F.log_softmax(x, -1), target, weight=w, ignore_index=R.IGNORE_LABEL)
    (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind", ["lazy", "cat", "identity", "tensor"])
@pytest.mark.parametrize("K", [1, 13, 20, 64])
def test_view_nll_against_float64(K, kind, dtype, weighted):
    case = R.view_case(K, seed=K)
    weight = case["weight"] if weighted else None
    x_view, leaf, materialise = view_inputs(case, kind, dtype)
    w_dev = None if weight is None else weight.to(DEV)
    loss = ops.view_nll(x_view, case["labels"].to(DEV), case["csr_idx"].to(DEV), weight=w_dev)
    assert loss.dtype == torch.float32 and loss.shape == ()
    (g,) = torch.autograd.grad(loss, leaf)
    assert g.dtype == dtype and g.shape == leaf.shape
    # float64 and float32 evaluations of the materialised formula, on the same rounded rows; their gradients are
    # brought to the leaf by autograd through the same gather
    rounded = leaf.detach().cpu().to(dtype)
    def reference(prec):
        r = rounded.to(prec).requires_grad_()
        mat = materialise(r)
        lab = case["labels"].clone()
        lab[(lab < 0) | (lab >= K)] = R.IGNORE_LABEL
        target = lab.repeat_interleave(case["csr_idx"][1:] - case["csr_idx"][:-1])
        w = None if weight is None else weight.to(prec)
        val = F.nll_loss(F.log_softmax(mat, -1), target, weight=w, ignore_index=R.IGNORE_LABEL)
        (grad,) = torch.autograd.grad(val, r)
        return val.detach(), grad
    l64, g64 = reference(torch.float64)
    l32, g32 = reference(torch.float32)
    restated = R.view_nll_ref(materialise(rounded), case["labels"], case["csr_idx"], weight)
    assert abs(float(restated) - float(l64)) <= 1e-12 * max(abs(float(l64)), 1e-30)
    rep = T.Report(f"view_nll K={K} {kind} {dtype} weighted={weighted}")
    rep.add("small", "loss", "out", T.rel_err(loss.reshape(1), l64.reshape(1)), T.rel_err(l32.reshape(1), l64.reshape(1)))
    if dtype == torch.float32:
        rep.add("small", "rows gradient", "grad_in", T.rel_err(g, g64), T.rel_err(g32, g64))
    else:
        # the gradient leaves in the rows' dtype: held to the float64 gradient rounded the same way, with the fp32
        # composition rounded the same way as the yardstick
        rep.add("small", "rows gradient", "grad_in", T.rel_err(g.float(), g64),
                T.rel_err(g32.to(dtype).float(), g64))
    rep.check()
    # rows that no counted view reads get exactly zero
    if kind in ("lazy", "cat"):
        assert bool((g[g64.to(DEV) == 0] == 0).all())
    # bitwise equality of two runs
    loss2 = ops.view_nll(x_view, case["labels"].to(DEV), case["csr_idx"].to(DEV), weight=w_dev)
    (g2,) = torch.autograd.grad(loss2, leaf)
    assert same_bits(loss.reshape(1), loss2.reshape(1)) and same_bits(g, g2)


@pytest.mark.parametrize("kind", ["lazy", "tensor"])
def test_view_nll_all_ignored_and_no_views(kind):
    K = 13
    case = R.view_case(K, seed=1)
    x_view, leaf, _ = view_inputs(case, kind, torch.float32)
    ignored = torch.full_like(case["labels"], R.IGNORE_LABEL).to(DEV)
    loss = ops.view_nll(x_view, ignored, case["csr_idx"].to(DEV))
    assert torch.isnan(loss)                                      # as torch: 0 / 0
    (g,) = torch.autograd.grad(loss, leaf)
    assert bool((g == 0).all())
    # an ignore_index of its own
    lab = case["labels"].clone()
    lab[lab == R.IGNORE_LABEL] = 255
    a = ops.view_nll(x_view, lab.to(DEV), case["csr_idx"].to(DEV), ignore_index=255)
    b = ops.view_nll(x_view, case["labels"].to(DEV), case["csr_idx"].to(DEV))
    assert same_bits(a.reshape(1), b.reshape(1))
    # V = 0
    n = 9
    csr0 = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    labels = torch.zeros(n, dtype=torch.int64, device=DEV)
    empty = torch.zeros(0, K, device=DEV, requires_grad=True)
    assert torch.isnan(ops.view_nll(empty, labels, csr0))
    rows = torch.randn(32, K, device=DEV, requires_grad=True)
    lazy = ops.GatheredFeatures(rows, torch.zeros(0, dtype=torch.int32, device=DEV),
                                torch.zeros(32, dtype=torch.int32, device=DEV), True)
    loss = ops.view_nll(lazy, labels, csr0)
    assert torch.isnan(loss)
    (g,) = torch.autograd.grad(loss, rows)
    assert bool((g == 0).all())


def test_view_nll_refuses_what_it_does_not_take():
    rows = torch.randn(8, 65, device=DEV)
    csr = torch.arange(9, device=DEV)
    labels = torch.zeros(8, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        ops.view_nll(rows, labels, csr)                                           # K > 64
    with pytest.raises(TypeError):
        ops.view_nll(rows[:, :13].double(), labels, csr)
    with pytest.raises(TypeError):
        ops.view_nll(rows[:, :13], labels.float(), csr)
    with pytest.raises(ValueError):
        ops.view_nll(rows[:, :13], labels, csr[:-1])
    with pytest.raises(ValueError):
        ops.view_nll(rows[:, :13], labels, csr, weight=torch.ones(5, device=DEV))


def test_view_nll_never_holds_a_view_sized_tensor():
    """V = 2^20 views of 2^14 rows, K = 20: forward + backward allocate less than ONE [V, K] float32 tensor (the
    materialised composition holds several) and nothing synchronises with the host."""
    V, Rn, K, n = 1 << 20, 1 << 14, 20, 1 << 16
    gen = torch.Generator().manual_seed(0)
    rows = torch.randn(Rn, K, generator=gen).to(DEV).requires_grad_()
    row_idx = torch.randint(0, Rn, (V,), generator=gen).int().to(DEV)
    csr = torch.arange(0, V + 1, V // n, dtype=torch.int64).to(DEV)
    labels = torch.randint(-1, K, (n,), generator=gen).to(DEV)
    lazy = ops.GatheredFeatures(rows, row_idx, torch.zeros(Rn, dtype=torch.int32, device=DEV), True)
    ops.view_nll(lazy, labels, csr).backward()                    # library load and workspace query
    rows.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = ops.view_nll(lazy, labels, csr)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < V * K * 4, (peak, V * K * 4)
    # and the value: the histogram of (row, label) pairs, in float64
    lp = torch.log_softmax(rows.detach().double(), -1)
    target = labels.repeat_interleave(V // n)
    keep = target >= 0
    want = -(lp[row_idx.long()[keep], target[keep]]).mean()
    assert T.rel_err(loss.reshape(1), want.reshape(1)) <= T.gate("out")


# ---------------------------------------------------------------------------------------------
# the tail
# ---------------------------------------------------------------------------------------------

def device_log_softmax(z):
    """The device's log-softmax of [N, K] logits, as a CPU tensor: the tail's row copies are held bit for bit against
    the restatement run on THESE values."""
    out, _ = ops.log_softmax_nll(z.to(DEV), torch.full((z.shape[0],), R.IGNORE_LABEL, dtype=torch.int64, device=DEV))
    return out.cpu()


@pytest.mark.parametrize("layout", ["f0.3", "none", "all", None])
@pytest.mark.parametrize("view_loss", [False, True])
@pytest.mark.parametrize("with_head", [False, True])
@pytest.mark.parametrize("training", [False, True])
def test_no3d_tail_against_the_restatement(training, with_head, view_loss, layout):
    K, C, n = 13, 32, 257
    case = R.view_case(K, seed=31)
    gen = torch.Generator().manual_seed(7)
    pos = R.uniform_cloud(n, seed=41)
    seen = None if layout is None else R.seen_layout(layout, pos, seed=42)
    labels = case["labels"].clone()
    labels[5] = 3
    width = C if with_head else K
    head = torch.nn.Sequential(torch.nn.Linear(C, K)) if with_head else None
    map_rows = torch.randn(case["rows"].shape[0], width, generator=gen)
    row_idx = case["row_idx"]
    if with_head:
        # output bit for bit "away from the head's matmul": both sides get the logits of the SAME (device) matmul
        features = torch.randn(n, C, generator=gen)
        head_dev = torch.nn.Sequential(torch.nn.Linear(C, K)).to(DEV)
        head_dev.load_state_dict(head.state_dict())
        with torch.no_grad():
            logits = head_dev(features.to(DEV)).cpu()
    else:
        features = torch.randn(n, K, generator=gen)
        logits = features
    view_c = (map_rows[row_idx.long()], case["csr_idx"]) if view_loss else None
    with torch.no_grad():
        want_out, _, want_labels = R.no3d_tail_ref(logits, seen, pos, labels, None, training, None,
                                                   log_softmax=device_log_softmax)
        _, want_loss, _ = R.no3d_tail_ref(features.double(), seen, pos, labels,
                                          None if head is None else head.double(), training,
                                          None if view_c is None else (view_c[0].double(), view_c[1]),
                                          dtype=torch.float64)
        _, loss32, _ = R.no3d_tail_ref(features, seen, pos, labels, None if head is None else head.float(), training,
                                       view_c)
    rows_dev = map_rows.to(DEV).requires_grad_()
    lazy = ops.GatheredFeatures(rows_dev, row_idx.to(DEV), torch.zeros(rows_dev.shape[0], dtype=torch.int32, device=DEV),
                                True)
    labels_dev = labels.to(DEV)
    before = labels_dev.clone()
    feats_dev = features.to(DEV).requires_grad_()
    out, loss = no3d.no3d_tail(feats_dev, None if seen is None else seen.to(DEV), pos.to(DEV), labels_dev,
                               head_dev if with_head else None, training,
                               (lazy, case["csr_idx"].to(DEV)) if view_loss else None)
    assert torch.equal(labels_dev, before), "the caller's labels are left as they are"
    assert out.dtype == torch.float32 and out.shape == (n, K)
    assert same_bits(out.detach().cpu(), want_out)
    if torch.isnan(want_loss):
        assert torch.isnan(loss)
        return
    err32 = T.rel_err(loss32.reshape(1), want_loss.reshape(1))
    assert T.rel_err(loss.reshape(1), want_loss.reshape(1)) <= T.gate("out", err32), (float(loss), float(want_loss))
    if training or view_loss:
        leaf = rows_dev if view_loss else feats_dev
        (g,) = torch.autograd.grad(loss, leaf)
        assert g.shape == leaf.shape and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    # without labels there is no loss
    out2, none = no3d.no3d_tail(features.to(DEV), None if seen is None else seen.to(DEV), pos.to(DEV), None,
                                head_dev if with_head else None, training)
    assert none is None and same_bits(out2.detach().cpu(), want_out)


def test_view_logits_keeps_a_lazy_gather_lazy_under_a_linear_head():
    rows = torch.randn(64, 32, device=DEV)
    idx = torch.randint(0, 64, (300,), device=DEV).int()
    lazy = ops.GatheredFeatures(rows, idx, torch.zeros(64, dtype=torch.int32, device=DEV), True)
    head = torch.nn.Sequential(torch.nn.Linear(32, 13)).to(DEV)
    got = no3d.view_logits(head, lazy)
    assert isinstance(got, ops.GatheredFeatures) and got.rows.shape == (64, 13) and got.row_idx is lazy.row_idx
    torch.testing.assert_close(got.materialize(), head(lazy.materialize()), rtol=1e-5, atol=1e-5)
    mlp = torch.nn.Sequential(torch.nn.Linear(32, 13), torch.nn.ReLU()).to(DEV)
    assert torch.is_tensor(no3d.view_logits(mlp, lazy))
    assert no3d.view_logits(None, lazy) is lazy


def branch_last_view(lazy_switch, training=False, drop_mod=0):
    """last_view_x_mod of a UnimodalBranch with keep_last_view over an exact nearest mapping."""
    from deepviewagg_amd.modules.multimodal import modules as M
    from deepviewagg_amd.modules.multimodal import pooling as P
    from deepviewagg_amd.modules.multimodal.fusion import BimodalFusion
    gen = torch.Generator().manual_seed(3)
    n, C, B, H, W = 40, 16, 2, 8, 8
    sizes = torch.randint(0, 4, (n,), generator=gen)
    csr = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)]).to(DEV)
    V = int(csr[-1])
    images = torch.randint(0, B, (V,), generator=gen).to(DEV)
    pixels = torch.stack([torch.randint(0, W, (V,), generator=gen), torch.randint(0, H, (V,), generator=gen)], 1).short()
    x = torch.randn(B, C, H, W, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last)
    atom_ptr = torch.arange(V + 1, device=DEV)
    lazy = ops.lazy_gather_nearest(x, ops.pack_gather_index(images, atom_ptr, pixels.to(DEV)), exact=True)

    class ModData:
        x = torch.zeros(1, 1)
        atomic_csr_indexing = atom_ptr
        view_csr_indexing = csr
        mapping_features = torch.zeros(V, 1, device=DEV)

        def get_mapped_features(self, interpolate=False):
            return lazy

    branch = M.UnimodalBranch(None, P.BimodalCSRPool(mode='max'), P.BimodalCSRPool(mode='max'),
                              BimodalFusion(mode='residual'), keep_last_view=True, drop_mod=drop_mod)
    branch.train(training)
    old = M.UnimodalBranch.KEEP_LAST_VIEW_LAZY
    M.UnimodalBranch.KEEP_LAST_VIEW_LAZY = lazy_switch
    try:
        out = branch({'x_3d': torch.zeros(n, C, device=DEV), 'x_seen': None, 'modalities': {'image': ModData()}}, 'image')
    finally:
        M.UnimodalBranch.KEEP_LAST_VIEW_LAZY = old
    return out['modalities']['image'].last_view_x_mod, lazy


def test_keep_last_view_lazy_switch():
    kept, lazy = branch_last_view(True)
    assert isinstance(kept, ops.GatheredFeatures) and kept.rows.shape[0] == lazy.rows.shape[0]
    plain, lazy = branch_last_view(False)
    assert torch.is_tensor(plain) and torch.equal(plain, lazy.materialize())
    # nn.Dropout in eval mode is the identity: the gather stays lazy; in training the dropout needs the [V, C] tensor
    kept, _ = branch_last_view(True, training=False, drop_mod=0.5)
    assert isinstance(kept, ops.GatheredFeatures)
    dropped, lazy = branch_last_view(True, training=True, drop_mod=0.5)
    assert torch.is_tensor(dropped) and dropped.shape == lazy.shape
