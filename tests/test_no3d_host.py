"""No GPU: the host side of the image-only model tail (deepviewagg_amd/models/no3d.py, csrc/nearest_seen.hip,
csrc/view_loss.hip): the restatements of tests/no3d_ref.py against torch, the argument checks of the C ABI, the drop-in
binding, and the margin cap behind the float64 cross-check of tests/test_gpu_no3d.py."""
import ctypes
import sys
import types

import pytest
import torch
import torch.nn.functional as F

import no3d_ref as R
from deepviewagg_amd import _lib

FAKE = ctypes.c_void_p(4096)        # never dereferenced: every call below returns before a launch


@pytest.mark.parametrize("K", [1, 13, 64])
@pytest.mark.parametrize("weighted", [False, True])
def test_view_loss_restatement_is_log_softmax_plus_nll(K, weighted):
    c = R.view_case(K, seed=K)
    x_view = c["rows"][c["row_idx"].long()].double()
    labels = c["labels"].clone()
    labels[5] = R.IGNORE_LABEL                    # torch asserts on an out-of-range target; the restatement skips it
    w = c["weight"].double() if weighted else None
    target = labels.repeat_interleave(c["csr_idx"][1:] - c["csr_idx"][:-1])
    want = F.nll_loss(F.log_softmax(x_view, -1), target, weight=w, ignore_index=R.IGNORE_LABEL)
    got = R.view_nll_ref(x_view, c["labels"], c["csr_idx"], w, R.IGNORE_LABEL, torch.float64)
    assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want))
    all_ignored = torch.full_like(labels, R.IGNORE_LABEL)
    assert torch.isnan(R.view_nll_ref(x_view, all_ignored, c["csr_idx"], w))


def test_nearest_seen_restatement_small_by_hand():
    pos = torch.tensor([[0., 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [1, 0, 0]])
    seen = torch.tensor([False, True, False, True, True])
    # point 0 -> 1 (tie of 1 and 4 at distance 1: the lower index); point 2 -> tie of 1, 3, 4: index 1
    assert R.nearest_seen_ref(pos, seen).tolist() == [1, 1, 1, 3, 4]
    assert R.nearest_seen_ref(pos, torch.zeros(5, dtype=torch.bool)).tolist() == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("with_head", [False, True])
@pytest.mark.parametrize("view_loss", [False, True])
@pytest.mark.parametrize("layout", ["f0.5", "none"])
def test_tail_restatement_against_torch(training, with_head, view_loss, layout):
    """The restatement against the same forward composed from torch's own pieces (F.log_softmax, F.nll_loss, an index
    assignment from a float64-free brute force): small case, every branch of no3d.py:105-154."""
    K, C, n = 13, 8, 257
    c = R.view_case(K, seed=21)
    gen = torch.Generator().manual_seed(5)
    pos = R.uniform_cloud(n, seed=11)
    seen = R.seen_layout(layout, pos, seed=12)
    head = torch.nn.Sequential(torch.nn.Linear(C, K)) if with_head else None
    width = C if with_head else K
    features = torch.randn(n, width, generator=gen)
    labels = c["labels"].clone()
    labels[5] = 2
    view_features = torch.randn(int(c["csr_idx"][-1]), width, generator=gen)
    view = (view_features, c["csr_idx"]) if view_loss else None
    before = labels.clone()
    with torch.no_grad():
        out, loss, masked = R.no3d_tail_ref(features, seen, pos, labels, head, training, view)
        assert torch.equal(labels, before)
        # the same, from torch's pieces
        logits = head(features) if with_head else features
        want_out = F.log_softmax(logits, -1)
        want_labels = labels.clone()
        if not training and bool(seen.any()):
            d = torch.stack([((pos[i] - pos[seen]) ** 2) for i in range(n)])          # [n, S, 3]
            d = (d[..., 0] + d[..., 1]) + d[..., 2]
            nn_idx = torch.stack([torch.nonzero(row == row.min())[0, 0] for row in d])
            want_out[~seen] = want_out[seen][nn_idx[~seen]]
        else:
            want_labels[~seen] = R.IGNORE_LABEL
        if view_loss:
            v_logits = head(view_features) if with_head else view_features
            target = want_labels.repeat_interleave(c["csr_idx"][1:] - c["csr_idx"][:-1])
            want = F.nll_loss(F.log_softmax(v_logits, -1), target, ignore_index=R.IGNORE_LABEL)
        else:
            want = F.nll_loss(want_out, want_labels, ignore_index=R.IGNORE_LABEL)
    assert torch.equal(out, want_out)
    assert torch.equal(masked, want_labels)
    if torch.isnan(want):
        assert torch.isnan(loss)
    else:
        assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want))


def test_abi_rejects_bad_arguments_without_gpu():
    lib = _lib.load()
    assert lib.dva_version() >= 326
    ns = lambda **kw: lib.dva_nearest_seen(*[kw.get(k, d) for k, d in (
        ("pos", FAKE), ("seen", FAKE), ("n", 8), ("bbox", FAKE), ("cell", 0.5), ("max_shell", 2), ("last", 1),
        ("done", FAKE), ("src", FAKE), ("any_seen", FAKE), ("x", None), ("K", 0), ("dtype", 0), ("filled", None),
        ("ws", FAKE), ("ws_bytes", 1 << 30), ("stream", None))])
    for name in ("pos", "seen", "bbox", "done", "src", "any_seen", "ws"):
        assert ns(**{name: None}) == -1, name                                          # null pointers
    assert ns(n=-1) == -1 and ns(cell=0.0) == -1 and ns(cell=float("nan")) == -1 and ns(max_shell=0) == -1
    assert ns(ws_bytes=16) == -1                                                       # workspace too small
    assert ns(x=FAKE) == -1 and ns(filled=FAKE) == -1                                  # rows in without rows out
    other = ctypes.c_void_p(8192)
    assert ns(x=FAKE, filled=other, K=0) == -1 and ns(x=FAKE, filled=other, K=13, dtype=7) == -1
    assert ns(x=FAKE, filled=FAKE, K=13) == -1                                         # filled aliases x
    assert ns(x=FAKE, filled=other, K=13, last=0) == -1                                # rows only with the last call
    assert ns(x=FAKE, filled=other, K=(1 << 20) + 1) == -2
    assert ns(n=1 << 30) == -2
    assert ns(n=0, pos=None, seen=None, src=None, done=None, ws=None) == 0             # an empty cloud is a no-op
    assert lib.dva_nearest_seen_workspace_bytes(-1) == -1
    assert lib.dva_nearest_seen_workspace_bytes(1 << 30) == -2
    assert lib.dva_nearest_seen_workspace_bytes(0) == 256
    assert lib.dva_nearest_seen_workspace_bytes(100) >= 100 * (8 + 4 + 8 + 4 + 16)      # keys, ids, their sorted twins, points

    counts = lambda **kw: lib.dva_view_nll_counts(*[kw.get(k, d) for k, d in (
        ("row_idx", FAKE), ("V", 8), ("csr", FAKE), ("labels", FAKE), ("N", 4), ("ignore", -1), ("R", 16), ("K", 13),
        ("cnt", FAKE), ("stream", None))])
    assert counts(cnt=None) == -1 and counts(csr=None) == -1 and counts(labels=None) == -1
    assert counts(V=-1) == -1 and counts(N=-1) == -1 and counts(R=-1) == -1 and counts(K=0) == -1
    assert counts(K=65) == -2 and counts(R=1 << 31, K=1) == -2 and counts(V=1 << 31) == -2
    assert counts(R=0, cnt=None) == 0
    fwd = lambda **kw: lib.dva_view_nll_fwd(*[kw.get(k, d) for k, d in (
        ("rows", FAKE), ("dtype", 0), ("cnt", FAKE), ("weight", None), ("R", 16), ("K", 13), ("loss", FAKE),
        ("numden", FAKE), ("ws", FAKE), ("ws_bytes", 1 << 20), ("stream", None))])
    for name in ("rows", "cnt", "loss", "numden", "ws"):
        assert fwd(**{name: None}) == -1, name
    assert fwd(R=-1) == -1 and fwd(K=0) == -1 and fwd(dtype=3) == -1 and fwd(ws_bytes=8) == -1
    assert fwd(K=65) == -2 and fwd(R=1 << 27, K=16) == -2
    bwd = lambda **kw: lib.dva_view_nll_bwd(*[kw.get(k, d) for k, d in (
        ("rows", FAKE), ("dtype", 0), ("cnt", FAKE), ("weight", None), ("numden", FAKE), ("g", FAKE), ("R", 16),
        ("K", 13), ("out", FAKE), ("stream", None))])
    for name in ("rows", "cnt", "numden", "g", "out"):
        assert bwd(**{name: None}) == -1, name
    assert bwd(R=-1) == -1 and bwd(K=0) == -1 and bwd(dtype=-1) == -1 and bwd(K=65) == -2
    assert bwd(R=0, rows=None, out=None) == 0
    assert lib.dva_view_nll_workspace_bytes() == 1024 * 2 * 8


def test_ops_refuse_host_tensors_and_bad_shapes():
    from deepviewagg_amd import ops
    pos, seen = torch.zeros(4, 3), torch.ones(4, dtype=torch.bool)
    with pytest.raises(_lib.DvaError):
        ops.nearest_seen(pos, seen)
    with pytest.raises(_lib.DvaError):
        ops.fill_unseen(torch.zeros(4, 13), pos, seen)
    with pytest.raises(_lib.DvaError):
        ops.view_nll(torch.zeros(4, 13), torch.zeros(2, dtype=torch.int64), torch.tensor([0, 2, 4]))
    with pytest.raises(TypeError):
        ops.view_nll([1, 2], torch.zeros(2, dtype=torch.int64), torch.tensor([0, 2, 4]))


def test_dropin_rebinds_no3d_forward():
    """install() rebinds No3D.forward of a loaded reference module and aliases the rest as tests/test_dropin.py expects."""
    for k in [k for k in sys.modules if k.startswith("torch_points3d")]:
        del sys.modules[k]
    from deepviewagg_amd import dropin
    from deepviewagg_amd.models import no3d
    try:
        name = "torch_points3d.models.segmentation.multimodal.no3d"
        parts = name.split(".")
        for i in range(1, len(parts) + 1):
            m = types.ModuleType(".".join(parts[:i]))
            m.__path__ = []
            sys.modules[m.__name__] = m

        class No3D:
            def forward(self, *args, **kwargs):
                raise AssertionError("the reference's forward (it imports pykeops)")

        class No3DImageLogitFusion(No3D):
            pass

        fake = sys.modules[name]
        fake.No3D, fake.No3DImageLogitFusion = No3D, No3DImageLogitFusion
        names = dropin.install(patch_existing=False)
        assert No3D.forward is no3d.forward and No3DImageLogitFusion.forward is no3d.forward
        assert name not in names and name not in dropin._ALIASES
        assert sys.modules[name] is fake
        assert "torch_points3d.modules.multimodal.pooling" in names and len(names) == len(dropin._ALIASES)
        import importlib
        from deepviewagg_amd.modules.multimodal import modules as our_modules
        assert importlib.import_module("torch_points3d.modules.multimodal.modules") is our_modules
    finally:
        for k in [k for k in sys.modules if k.startswith("torch_points3d")]:
            del sys.modules[k]
    # without the module nothing happens, silently
    assert dropin.install(patch_existing=False)
    assert "torch_points3d.models.segmentation.multimodal.no3d" not in sys.modules
    for k in [k for k in sys.modules if k.startswith("torch_points3d")]:
        del sys.modules[k]


def test_keep_last_view_lazy_is_off_by_default():
    from deepviewagg_amd.modules.multimodal.modules import UnimodalBranch
    assert UnimodalBranch.KEEP_LAST_VIEW_LAZY is False


def test_margin_cap_of_the_float64_cross_check():
    """tests/test_gpu_no3d.py holds src to the float64 brute force on every query of the uniform clouds whose two nearest
    float64 squared distances differ by more than 1e-4 relative.  That check is worth something only while few queries
    fall inside the margin: at most 1 % per cloud (measured: 0 - 0.61 %)."""
    worst = 0.0
    for name, pos, seen in R.uniform_cases():
        q = int((~seen).sum())
        if q == 0 or int(seen.sum()) == 0:
            continue
        _, d1, d2 = R.nearest_seen_ref(pos, seen, torch.float64, with_margin=True)
        share = float(R.in_margin(d1, d2)[~seen].sum()) / q
        worst = max(worst, share)
        assert share <= 0.01, (name, share)
    print(f"largest share of queries inside the margin: {100 * worst:.3f} %")
