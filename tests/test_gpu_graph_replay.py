"""-m gpu: the pooling step, the losses and the other ops that promise no host read, captured once in a
``torch.cuda.CUDAGraph`` and replayed on new contents of the same buffers, against an eager twin (tests/graph_replay.py;
DESIGN.md "Graph replay").  One capture per test.  The gate is measured, not typed in: 4 x the twin's own run-to-run
spread per tensor, bit for bit where that spread is 0.  The pooling cases anchor the output of the last replay to the
CPU oracle with the gate of the path's own test file as well.

Content sets of every pooling case (the same buffers, the same ``csr``): the case's own; new feature maps with the
signs flipped and one map all zero, and new mapping features (the arg-max view of the DeepSet pool moves); every
parameter x 4; new ``images`` and ``pixels`` in place (the row plan is built inside the step and must follow).

The eager gradients are order-noisy and some are two-valued between runs (DESIGN.md "Graph replay" has the measured
figures); the harness samples the twin 20 times per content set, and further where a row still misses, before it judges."""
import contextlib

import numpy as np
import pytest
import torch

import graph_replay as GR
import test_gpu_bilinear as TB
import test_gpu_chain as TC
import test_gpu_qkv_chain as TQ
from oracle import pooling_oracle as O
from test_gpu_chain import check_plan_kind, plan_kind, ragged_long, rel          # noqa: F401  (plan_kind: a fixture)
from tolerances import gate, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@contextlib.contextmanager
def patched(obj, **attrs):
    old = {k: getattr(obj, k) for k in attrs}
    for k, v in attrs.items():
        setattr(obj, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(obj, k, v)


@contextlib.contextmanager
def counted(obj, name, calls):
    real = getattr(obj, name)

    def spy(*a, **k):
        calls[name] = calls.get(name, 0) + 1
        return real(*a, **k)
    with patched(obj, **{name: spy}):
        yield


# ---------------------------------------------------------------------------------------------------------------
# pooling: forward + backward of one module on a lazy gather, everything from the index packing on inside the step
# ---------------------------------------------------------------------------------------------------------------

class Pool:
    """One pooling case: the CPU inputs, the oracle module and its state, and ``make()`` = (step, statics) on fresh
    device tensors and a fresh device module (called twice: the captured side and the eager twin)."""

    def __init__(self, case, builder, bf16, train=True, qkv=False, bilinear=False, w=None):
        self.case, self.builder, self.bf16, self.train, self.qkv, self.bilinear = case, builder, bf16, train, qkv, bilinear
        self.ref, _ = builder()
        self.sd = {k: v.clone() for k, v in self.ref.state_dict().items()}
        self.params = [n for n, _ in self.ref.named_parameters()]
        self.w = case["w"] if w is None else w
        self.x_main = torch.randn(case["N"], 6, generator=case["gen"]) if qkv else None
        self.used = {}

    def state(self):
        return {"m." + k: v for k, v in self.sd.items()}

    def make(self):
        from deepviewagg_amd import ops
        from deepviewagg_amd.modules.multimodal import pooling as P
        case, train = self.case, self.train
        _, m = self.builder()
        V = case["V"]
        x = case["x"].to(DEV)
        if self.bf16:
            x = x.bfloat16().contiguous(memory_format=torch.channels_last)
        x.requires_grad_(train)
        s = dict(x=x, images=case["images"].to(DEV), pixels=case["pixels"].to(DEV), x_map=case["x_map"].to(DEV),
                 w=self.w.to(DEV))
        if self.qkv:
            s["x_main"] = self.x_main.to(DEV).requires_grad_(train)
        for k, t in list(m.named_parameters()) + list(m.named_buffers()):
            s["m." + k] = t
        assert set(self.state()) <= set(s)
        csr, atom_ptr = case["csr"].to(DEV), torch.arange(V + 1, device=DEV)
        atomic_pool = P.BimodalCSRPool(mode='max')
        res_m1 = None
        if self.bilinear:
            res_m1 = (torch.tensor([case["msize"]], dtype=torch.float32) - 1).to(DEV)
        used = self.used

        def forward():
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.bf16):
                packed = ops.pack_gather_index(s["images"], atom_ptr, s["pixels"])
                if self.bilinear:
                    coords = (s["pixels"] / res_m1).flip(1)                    # (row, col) in [0, 1]
                    lazy = ops.lazy_gather_bilinear(x, packed, coords, exact=True)
                else:
                    lazy = ops.lazy_gather_nearest(x, packed, exact=True)
                lazy = atomic_pool(None, lazy, None, atom_ptr)
                return m(s.get("x_main"), lazy, s["x_map"], csr)

        def step():
            if not train:
                with torch.no_grad():
                    return {"out": forward()}
            out = forward()
            used["fn"] = type(out.grad_fn).__name__
            (out.float() * s["w"]).sum().backward()
            return {"out": out}
        return step, s

    def contents(self, seed=101):
        case = self.case
        gen = torch.Generator().manual_seed(seed)
        V, x = case["V"], case["x"]
        B = x.shape[0]
        wmax, hmax = case.get("msize", (x.shape[3], x.shape[2]))
        base = dict(x=x, x_map=case["x_map"], images=case["images"], pixels=case["pixels"])
        x1 = -torch.randn(x.shape, generator=gen).bfloat16().float()
        x1[1] = 0.0
        c1 = dict(base, x=x1, x_map=torch.rand(V, 8, generator=gen))
        c2 = dict(base, **{"m." + n: 4.0 * self.sd[n] for n in self.params})
        pixels = torch.stack([torch.randint(0, wmax, (V,), generator=gen),
                              torch.randint(0, hmax, (V,), generator=gen)], 1).short()
        c3 = dict(base, x=-x, images=torch.randint(0, B, (V,), generator=gen), pixels=pixels,
                  x_map=torch.rand(V, 8, generator=gen))
        return [base, c1, c2, c3]

    def oracle_out(self, c, dtype=torch.float32, autocast=False):
        """The CPU oracle's output on content set ``c`` (the module's own state)."""
        import copy
        ref = copy.deepcopy(self.ref).to(dtype)
        ref.load_state_dict({k: (v.to(dtype) if v.is_floating_point() else v) for k, v in self.sd.items()})
        ref.train(self.train)
        x = c["x"].to(dtype)
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            if self.bilinear:
                x_mod = O.gather_bilinear(x, c["images"], c["pixels"], self.case["msize"])
            else:
                x_mod = O.gather_nearest(x, c["images"], c["pixels"])
            x_main = None if self.x_main is None else self.x_main.to(dtype)
            return ref(x_main, x_mod, c["x_map"].to(dtype), self.case["csr"])

    def run(self, title):
        contents = self.contents()
        step, statics = self.make()
        res = GR.run_replay(step, statics, contents, state=self.state(), twin=self.make(), title=title)
        assert len(res.replayed) == len(contents) + 1
        last = res.replayed[-1]
        out = last["out:out"]
        # the running statistics moved in place, and by one step only (the state is restored before every replay)
        if self.train:
            moved = [k for k in last if "running_mean" in k and not torch.equal(last[k].cpu(), self.sd[k[2:]])]
            assert moved, "no running_mean moved: the statistics were not updated in place"
            for k in last:
                if k.endswith("num_batches_tracked"):
                    assert int(last[k]) == int(self.sd[k[2:]]) + 1, (k, int(last[k]))
        # anchor: the last replay against the CPU oracle, with the gate of the path's own test file
        c = contents[-1]
        if self.bf16:
            assert out.dtype == torch.bfloat16
            out_ref = self.oracle_out(c)
            r, r_amp = rel(out, out_ref), rel(self.oracle_out(c, autocast=True), out_ref)
            print(f"{title}: last replay against the oracle, rel L2 {r:.4f} (oracle under autocast {r_amp:.4f})")
            assert r < max(2e-2, 1.5 * r_amp), (r, r_amp)
        else:
            out64 = self.oracle_out(c, torch.float64)
            e, e32 = rel_err(out, out64), rel_err(self.oracle_out(c), out64)
            print(f"{title}: last replay against float64, err {e:.2e} (oracle in fp32 {e32:.2e}, gate {gate('out', e32):.2e})")
            assert e <= gate("out", e32), (e, e32)
        unseen = self.case["csr"][1:] == self.case["csr"][:-1]
        assert float(out.float().cpu()[unseen].abs().max() if unseen.any() else 0.0) == 0.0
        return res


@contextlib.contextmanager
def chain_forced():
    from deepviewagg_amd import fused_chain
    with patched(fused_chain, FORCE=True):
        yield


@pytest.mark.parametrize("N,C,G,gating,scaling", [(2000, 64, 4, True, True), (1500, 32, 2, False, False)])
def test_bf16_chain_train(N, C, G, gating, scaling, plan_kind):
    """GroupBimodalCSRPool on the bf16 recompute chain, lazy nearest gather as in test_gpu_chain.run_dev, over both row
    plans (the split plan is what the headline runs); the second case has no gate and no group scaling (NULL gate
    pointers)."""
    case = TC.make_case(31, N, C, ragged_long)
    pool = Pool(case, lambda: TC.build(case, G, True, gating=gating, scaling=scaling), bf16=True)
    with chain_forced():
        pool.run(f"bf16 chain C={C} G={G} N={N} {'gate' if gating else 'no gate'} {plan_kind['kind'][:5]}")
    check_plan_kind(plan_kind, C)


@pytest.mark.parametrize("one_kernel", [True, False])
def test_qkv_chain_train(one_kernel):
    from deepviewagg_amd import fused_chain
    case = TC.make_case(33, 2000, 64, ragged_long)
    pool = Pool(case, lambda: TQ.build(case, 4, 8, True), bf16=True, qkv=True)
    calls = {}
    with patched(fused_chain, QKV_ONE_KERNEL=one_kernel), counted(fused_chain, "qkv_pool", calls), \
            counted(fused_chain, "qkv_compatibilities", calls):
        pool.run(f"QKV chain C=64 G=4 qk=8 N=2000 {'one kernel' if one_kernel else 'keys + scores-in attention'}")
    assert calls.get("qkv_pool" if one_kernel else "qkv_compatibilities", 0) >= 1, calls
    assert calls.get("qkv_compatibilities" if one_kernel else "qkv_pool", 0) == 0, calls


@pytest.mark.parametrize("path", ["chain_f32", "stored"])
def test_fp32_train(path):
    """fp32, no autocast: the recompute chain (fused_chain_f32) and, with it disabled, the stored-activation DeepSet
    kernels."""
    from deepviewagg_amd import fused_chain_f32, fused_deepset
    case = TC.make_case(35, 1500, 32, ragged_long)
    pool = Pool(case, lambda: TC.build(case, 2, True), bf16=False)
    calls = {}
    with patched(fused_chain_f32, ENABLED=(path == "chain_f32")), counted(fused_chain_f32, "chain_scores", calls), \
            counted(fused_deepset, "deepset_linear", calls):
        pool.run(f"fp32 {path} C=32 G=2 N=1500")
    assert calls.get("chain_scores" if path == "chain_f32" else "deepset_linear", 0) >= 1, calls
    assert calls.get("deepset_linear" if path == "chain_f32" else "chain_scores", 0) == 0, calls


def test_fused_bilinear_train():
    sizes_fn, N, C_in, C_out, G, train = min((c for c in TB.CASES if c[5]), key=lambda c: (c[1], c[2] * c[3]))
    case = TB.make_case(37, N, C_in, sizes_fn)
    w = torch.randn(N, C_out, generator=case["gen"])
    pool = Pool(case, lambda: TB.build(case, C_out, G, True), bf16=True, bilinear=True, w=w)
    pool.run(f"fused bilinear {sizes_fn.__name__} N={N} {C_in}->{C_out} G={G}")
    assert pool.used["fn"] == "_EmodPoolBackward", f"the fused bilinear path must be the one that ran ({pool.used})"


def test_bf16_chain_eval_forward():
    """Eval mode under no_grad: the single fused launch."""
    case = TC.make_case(39, 2000, 64, ragged_long)
    pool = Pool(case, lambda: TC.build(case, 4, False), bf16=True, train=False)
    with chain_forced():
        pool.run("bf16 chain eval C=64 G=4 N=2000")


# ---------------------------------------------------------------------------------------------------------------
# the ops that promise no host read
# ---------------------------------------------------------------------------------------------------------------
P_SEG, C_SEG, IGNORE = 1025, 13, -1


def _seg_labels(gen):
    return torch.randint(-1, C_SEG, (P_SEG,), generator=gen)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_log_softmax_nll(dtype):
    from deepviewagg_amd import ops

    def make():
        gen = torch.Generator().manual_seed(41)
        s = dict(logits=(2 * torch.randn(P_SEG, C_SEG, generator=gen)).to(DEV, dtype).requires_grad_(),
                 labels=_seg_labels(gen).to(DEV), weight=(torch.rand(C_SEG, generator=gen) + 0.5).to(DEV),
                 up=(torch.randn(P_SEG, C_SEG, generator=gen) / P_SEG).to(DEV))

        def step():
            logp, loss = ops.log_softmax_nll(s["logits"], s["labels"], s["weight"], ignore_index=IGNORE)
            (loss + (logp * s["up"]).sum()).backward()
            return {"logp": logp, "loss": loss}
        return step, s
    gen = torch.Generator().manual_seed(42)
    contents = [dict(logits=2 * torch.randn(P_SEG, C_SEG, generator=gen), labels=_seg_labels(gen),
                     weight=torch.rand(C_SEG, generator=gen) + 0.5) for _ in range(3)]
    contents[1]["labels"] = torch.full((P_SEG,), IGNORE)              # every label ignored: the loss is NaN in both runs
    step, statics = make()
    res = GR.run_replay(step, statics, contents, twin=make(), title=f"log_softmax_nll {dtype}")
    losses = [float(r["out:loss"]) for r in res.replayed]
    assert np.isnan(losses[2]) and not np.isnan(losses[0]) and not np.isnan(losses[3]), losses
    assert res.replayed[3]["logits.grad"].dtype == dtype


def test_lovasz_softmax_present():
    from deepviewagg_amd import ops

    def make():
        gen = torch.Generator().manual_seed(43)
        s = dict(probas=torch.softmax(2 * torch.randn(P_SEG, C_SEG, generator=gen), 1).to(DEV).requires_grad_(),
                 labels=_seg_labels(gen).to(DEV))

        def step():
            loss = ops.lovasz_softmax_flat(s["probas"], s["labels"], classes="present", ignore=IGNORE)
            loss.backward()
            return {"loss": loss}
        return step, s
    gen = torch.Generator().manual_seed(44)
    contents = [dict(probas=torch.softmax(2 * torch.randn(P_SEG, C_SEG, generator=gen), 1), labels=_seg_labels(gen))
                for _ in range(4)]
    lab = contents[1]["labels"]
    lab[(lab == 3) | (lab == 7)] = 0                                   # two classes leave: the mean runs over 11, not 13
    contents[2]["labels"] = torch.full((P_SEG,), IGNORE)              # every point ignored: loss 0, zero gradient
    step, statics = make()
    res = GR.run_replay(step, statics, contents, twin=make(), title="lovasz_softmax_flat present")
    assert float(res.replayed[3]["out:loss"]) == 0.0 and float(res.replayed[3]["probas.grad"].abs().max()) == 0.0
    assert float(res.replayed[4]["out:loss"]) > 0.0
    # the class-presence mask followed the labels: no gradient in the columns of the classes that left
    g = res.replayed[2]["probas.grad"]
    assert float(g[:, [3, 7]].abs().max()) == 0.0 and float(g[:, 0].abs().max()) > 0.0


def test_confusion_counts_accumulate():
    from deepviewagg_amd import ops

    def make():
        gen = torch.Generator().manual_seed(45)
        s = dict(outputs=torch.randn(P_SEG, C_SEG, generator=gen).to(DEV), labels=_seg_labels(gen).to(DEV),
                 counts=torch.zeros(C_SEG, C_SEG, dtype=torch.int64, device=DEV))

        def step():
            counts, n_bad = ops.confusion_counts(s["outputs"], s["labels"], C_SEG, ignore_index=IGNORE, out=s["counts"])
            assert counts is s["counts"]
            return {"n_bad": n_bad}
        return step, s
    gen = torch.Generator().manual_seed(46)
    contents = []
    for _ in range(3):
        labels = _seg_labels(gen)
        labels[torch.randint(0, P_SEG, (7,), generator=gen)] = C_SEG + 2         # outside [0, C): counted in n_bad
        contents.append(dict(outputs=torch.randn(P_SEG, C_SEG, generator=gen), labels=labels))
    step, statics = make()
    res = GR.run_replay(step, statics, contents, initial=dict(counts=torch.zeros(C_SEG, C_SEG, dtype=torch.int64)),
                        twin=make(), title="confusion_counts into a static matrix")
    # after k replays: the sum over the same k content sets (the harness holds every replay to the twin; independently:)
    seq = [contents[0]] + contents
    want = torch.zeros(C_SEG, C_SEG, dtype=torch.int64)
    bad = 0
    for c in seq:
        ok = (c["labels"] >= 0) & (c["labels"] < C_SEG)
        want.index_put_((c["labels"][ok], c["outputs"][ok].argmax(1)), torch.ones(int(ok.sum()), dtype=torch.int64),
                        accumulate=True)
        bad += int((c["labels"] >= C_SEG).sum())
    assert torch.equal(res.replayed[-1]["counts"].cpu(), want)
    assert sum(int(r["out:n_bad"]) for r in res.replayed) == bad and bad > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sparse_conv(dtype):
    """n = 1100 voxels, 32 -> 64 channels, k = 3; the kernel map is built before the capture (its spans are read on the
    host)."""
    from deepviewagg_amd import ops
    from test_gpu_sparseconv import _maps, surface_cloud
    n, cin, cout, k = 1100, 32, 64, 3
    coords = surface_cloud(n, 14, seed=n + 1)
    nbr, nbr_t = _maps(coords, k, 1)
    rows = coords.shape[0]

    def draw(gen, wscale=1.0):
        return dict(x=torch.randn(rows, cin, generator=gen),
                    W=wscale * torch.randn(k ** 3, cin, cout, generator=gen) / np.sqrt(cin * k ** 3 / 4),
                    b=torch.randn(cout, generator=gen), g=torch.randn(rows, cout, generator=gen))

    def make():
        c = draw(torch.Generator().manual_seed(47))
        s = dict(x=c["x"].to(DEV, dtype).requires_grad_(), W=c["W"].to(DEV).requires_grad_(),
                 b=c["b"].to(DEV).requires_grad_(), g=c["g"].to(DEV, dtype))

        def step():
            out = ops.sparse_conv(s["x"], s["W"], s["b"], nbr, nbr_t)
            out.backward(s["g"])
            return {"out": out}
        return step, s
    gen = torch.Generator().manual_seed(48)
    contents = [draw(gen), draw(gen, 4.0), draw(gen)]
    contents[2]["x"][::2] = 0.0
    step, statics = make()
    res = GR.run_replay(step, statics, contents, twin=make(), title=f"sparse_conv {dtype}")
    assert res.replayed[-1]["out:out"].dtype == dtype and res.replayed[-1]["W.grad"].dtype == torch.float32


def test_collate_mapping():
    """Three small mappings: new images, pixels and features at the same shapes.  The image offsets are maxima taken
    on the device, so they follow the new image ids."""
    from deepviewagg_amd import ops
    from mapping_collate_ref import collate_reference, make_mapping
    views = [np.array([2, 0, 3, 1, 40, 0]), np.array([1, 1, 0, 5]), np.array([0, 7, 2, 2, 0, 1, 3])]

    def draw(seed):
        rng = np.random.default_rng(seed)
        return [make_mapping(rng, v, atoms_per_view=[1, 2, 3], num_images=ni, feat=8) for v, ni in zip(views, (5, 2, 9))]

    def named(items):
        out = {}
        for b, (_, images, _, pixels, feats) in enumerate(items):
            out.update({f"images{b}": torch.from_numpy(images), f"pixels{b}": torch.from_numpy(pixels),
                        f"features{b}": torch.from_numpy(feats)})
        return out

    def make():
        items = draw(49)
        s = {k: v.to(DEV) for k, v in named(items).items()}
        fixed = [(torch.from_numpy(it[0]).to(DEV), torch.from_numpy(it[2]).to(DEV)) for it in items]

        def step():
            out = ops.collate_mapping([(p, s[f"images{b}"], a, s[f"pixels{b}"], s[f"features{b}"])
                                       for b, (p, a) in enumerate(fixed)])
            return dict(zip(("pointers", "images", "atom_ptr", "pixels", "features", "image_offsets"), out))
        return step, s
    drawn = [draw(50), draw(51), draw(52)]
    step, statics = make()
    res = GR.run_replay(step, statics, [named(d) for d in drawn], twin=make(), title="collate_mapping")
    ref = collate_reference(drawn[-1])
    for key in ("pointers", "images", "atom_ptr", "pixels", "image_offsets"):
        assert torch.equal(res.replayed[-1]["out:" + key].cpu(), torch.from_numpy(ref[key])), key
    assert torch.equal(res.replayed[-1]["out:features"].cpu().view(torch.int32),
                       torch.from_numpy(ref["features"]).view(torch.int32))


def test_vote_add_accumulates():
    from deepviewagg_amd import ops
    N, P, C = 300, 257, 13

    def draw(gen):
        ids = torch.randint(0, N, (P,), generator=gen)
        ids[:3] = torch.tensor([-1, N, N + 5])                                       # outside [0, N): n_bad
        return dict(ids=ids, outputs=torch.rand(P, C, generator=gen) * 8)

    def make():
        c = draw(torch.Generator().manual_seed(53))
        s = dict(votes=torch.zeros(N, C, device=DEV), counts=torch.zeros(N, dtype=torch.int32, device=DEV),
                 slots=ops.vote_slots(N, DEV), ids=c["ids"].to(DEV), outputs=c["outputs"].to(DEV))

        def step():
            return {"n_bad": ops.vote_add(s["votes"], s["counts"], s["ids"], s["outputs"], s["slots"])}
        return step, s
    gen = torch.Generator().manual_seed(54)
    contents = [draw(gen) for _ in range(3)]
    step, statics = make()
    zero = dict(votes=torch.zeros(N, C), counts=torch.zeros(N, dtype=torch.int32))
    res = GR.run_replay(step, statics, contents, initial=zero, twin=make(), title="vote_add into static votes")
    last = res.replayed[-1]
    assert bool((last["slots"] == -1).all()), "the slot array reads all -1 after every call"
    assert all(int(r["out:n_bad"]) == 3 for r in res.replayed)
    seen = torch.zeros(N, dtype=torch.int32)
    for c in [contents[0]] + contents:
        ok = c["ids"][(c["ids"] >= 0) & (c["ids"] < N)]
        seen[torch.unique(ok)] += 1                                                   # an id is counted once per call
    assert torch.equal(last["counts"].cpu(), seen)
