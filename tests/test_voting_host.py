"""Voting and K-NN interpolation without a GPU: the C-ABI argument checks of the dva_vote_* / dva_knn_interpolate
entries, the wrappers' refusal of CPU tensors, the drop-in name, and the CPU restatements of tests/voting_ref.py held
against torch's own forms of the same lines."""
import importlib
import sys

import numpy as np
import pytest
import torch

import voting_ref as R
from deepviewagg_amd import _lib


def test_abi_entries_reject_bad_arguments():
    lib = _lib.load()
    assert lib.dva_version() >= 315
    one, big, F32 = 1, 1 << 40, _lib.DVA_F32
    wsb = lib.dva_vote_workspace_bytes
    assert wsb(-1) == -1 and wsb(1 << 31) == -2
    assert wsb(0) >= 4 and wsb(300) >= 1200 and wsb(300) % 4 == 0
    add = lib.dva_vote_add
    #          votes counts N   C   ids  out  dtype P  slots bytes n_bad stream
    assert add(None, one, 300, 13, one, one, F32, 10, one, big, one, None) == -1
    assert add(one, None, 300, 13, one, one, F32, 10, one, big, one, None) == -1
    assert add(one, one, 300, 13, None, one, F32, 10, one, big, one, None) == -1
    assert add(one, one, 300, 13, one, None, F32, 10, one, big, one, None) == -1
    assert add(one, one, 300, 13, one, one, F32, 10, None, big, one, None) == -1
    assert add(one, one, 300, 13, one, one, F32, 10, one, big, None, None) == -1
    assert add(one, one, 300, 13, one, one, F32, 10, one, 8, one, None) == -1               # slot array too small
    assert add(one, one, 300, 13, one, one, 5, 10, one, big, one, None) == -1               # dtype
    assert add(one, one, -1, 13, one, one, F32, 10, one, big, one, None) == -1
    assert add(one, one, 300, 13, one, one, F32, -1, one, big, one, None) == -1
    assert add(one, one, 300, 0, one, one, F32, 10, one, big, one, None) == -1              # C = 0
    assert add(one, one, 300, 65, one, one, F32, 10, one, big, one, None) == -2             # C = 65
    assert add(one, one, 1 << 31, 13, one, one, F32, 10, one, big, one, None) == -2
    assert add(one, one, 300, 13, one, one, F32, 1 << 31, one, big, one, None) == -2        # a row position is int32
    assert add(one, one, 300, 13, None, None, F32, 0, one, big, one, None) == 0             # no rows: nothing to do
    itp = lib.dva_knn_interpolate
    #          x    M    C   nbr  d2   n   k  own   y    pred labels ign counts n_bad stream
    assert itp(None, 300, 13, one, one, 10, 3, None, one, None, None, -1, None, None, None) == -1
    assert itp(one, 300, 13, None, one, 10, 3, None, one, None, None, -1, None, None, None) == -1
    assert itp(one, 300, 13, one, None, 10, 3, None, one, None, None, -1, None, None, None) == -1
    assert itp(one, 300, 13, one, one, 10, 3, None, None, None, None, -1, None, None, None) == -1    # no output
    assert itp(one, 300, 13, one, one, 10, 3, None, None, one, None, -1, one, one, None) == -1       # counts, no labels
    assert itp(one, 300, 13, one, one, 10, 3, None, None, one, one, -1, one, None, None) == -1       # counts, no n_bad
    assert itp(one, -1, 13, one, one, 10, 3, None, one, None, None, -1, None, None, None) == -1
    assert itp(one, 300, 13, one, one, -1, 3, None, one, None, None, -1, None, None, None) == -1
    assert itp(one, 300, 13, one, one, 10, 0, None, one, None, None, -1, None, None, None) == -1     # k = 0
    assert itp(one, 300, 13, one, one, 10, -2, None, one, None, None, -1, None, None, None) == -1
    assert itp(one, 2, 13, one, one, 10, 3, None, one, None, None, -1, None, None, None) == -1       # k > M
    assert itp(one, 300, 0, one, one, 10, 3, None, one, None, None, -1, None, None, None) == -1      # C = 0
    assert itp(one, 300, 65, one, one, 10, 3, None, one, None, None, -1, None, None, None) == -2     # C = 65
    assert itp(one, 300, 13, one, one, 10, 129, None, one, None, None, -1, None, None, None) == -2   # k = 129
    assert itp(one, 300, 13, one, one, 1 << 30, 3, None, one, None, None, -1, None, None, None) == -2   # n k >= 2^31
    assert itp(one, 1 << 31, 13, one, one, 10, 3, None, one, None, None, -1, None, None, None) == -2
    assert itp(None, 300, 13, None, None, 0, 3, None, one, None, None, -1, None, None, None) == 0    # no queries


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from deepviewagg_amd import ops
    votes, counts = torch.zeros(5, 3), torch.zeros(5, dtype=torch.int32)
    ids, out, slots = torch.zeros(4, dtype=torch.int64), torch.zeros(4, 3), torch.full((64,), -1, dtype=torch.int32)
    x, pos_x, pos_y = torch.zeros(5, 3), torch.zeros(5, 3), torch.zeros(7, 3)
    for call in (lambda: ops.vote_add(votes, counts, ids, out, slots),
                 lambda: ops.knn_interpolate(x, pos_x, pos_y, k=3),
                 lambda: ops.knn_interpolate_labels(x, pos_x, pos_y, k=1)):
        with pytest.raises(_lib.DvaError, match="HIP device only"):          # the require_device policy
            call()
    for kw in ({"batch_x": torch.zeros(5, dtype=torch.int64)}, {"batch_y": torch.zeros(7, dtype=torch.int64)}):
        with pytest.raises(NotImplementedError, match="batch_x / batch_y"):
            ops.knn_interpolate(x, pos_x, pos_y, **kw)


def _clear():
    for k in [k for k in sys.modules if k.startswith("torch_points3d")]:
        del sys.modules[k]


@pytest.mark.parametrize("patch_existing", [False, True])
def test_dropin_alias_resolves(patch_existing):
    from deepviewagg_amd import dropin
    from deepviewagg_amd.metrics import segmentation_helpers as SH
    _clear()
    try:
        names = dropin.install(patch_existing=patch_existing)
        assert "torch_points3d.metrics.segmentation_helpers" in names
        mod = importlib.import_module("torch_points3d.metrics.segmentation_helpers")
        assert mod.SegmentationVoter is SH.SegmentationVoter
        from torch_points3d.metrics.segmentation_helpers import SegmentationVoter     # a tracker's own import line
        assert SegmentationVoter is SH.SegmentationVoter
    finally:
        _clear()


def test_voter_k_setter_keeps_the_reference_exceptions():
    from deepviewagg_amd.metrics.segmentation_helpers import SegmentationVoter
    voter = SegmentationVoter.__new__(SegmentationVoter)         # the setter needs no device
    voter._k = 1
    voter.k = 3
    assert voter.k == 3
    with pytest.raises(Exception, match="k should be >= 1"):
        voter.k = 0
    with pytest.raises(Exception, match="should be an int"):
        voter.k = 2.0
    assert voter.k == 3


def test_rank_loop_equals_the_index_add_form_bit_for_bit():
    """The restatement the GPU tests compare against is torch_geometric's own dataflow: M = 300, n = 257, k = 3,
    C = 13, 20 queries coinciding with search points (the 1e-16 clamp)."""
    g = torch.Generator().manual_seed(11)
    M, n, k, C = 300, 257, 3, 13
    pos_x = torch.rand(M, 3, generator=g)
    pos_y = torch.rand(n, 3, generator=g)
    pos_y[:20] = pos_x[torch.randperm(M, generator=g)[:20]]
    x = torch.rand(M, C, generator=g) * 64
    nbr, d2 = R.knn_ref(pos_y, pos_x, k)
    assert (d2[:20, 0] == 0).all() and (d2[20:, 0] > 0).all()
    loop = R.interpolate_ref(x, nbr, d2)
    form = R.interpolate_index_add_form(x, pos_x, pos_y, nbr)
    assert torch.equal(loop, form)
    assert torch.isfinite(loop).all()
    # a coinciding query takes the value of its search point up to the rounding of x w / w
    assert torch.allclose(loop[:20], x[torch.as_tensor(nbr[:20, 0]).long()], rtol=1e-6)
    # and the K-NN restatement is knn_bruteforce when the two clouds are one
    from oracle.knn_oracle import knn_bruteforce
    a, b = R.knn_ref(pos_x, pos_x, k), knn_bruteforce(pos_x.numpy(), k)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_vote_loop_equals_torch_on_duplicate_free_ids():
    g = torch.Generator().manual_seed(12)
    N, C, P = 300, 13, 257
    votes, counts = torch.zeros(N, C), torch.zeros(N, dtype=torch.int32)
    tv, tc = votes.clone(), counts.clone()
    for _ in range(2):
        ids = torch.randperm(N, generator=g)[:P]
        out = torch.rand(P, C, generator=g) * 8
        assert R.vote_add_ref(votes, counts, ids, out) == 0
        tv[ids] += out
        tc[ids] += 1
    assert torch.equal(votes, tv) and torch.equal(counts, tc) and int(counts.max()) == 2


def test_vote_loop_counts_the_last_occurrence_once():
    votes, counts = torch.zeros(4, 2), torch.zeros(4, dtype=torch.int32)
    ids = torch.tensor([1, 3, 1, -1, 4, 1])
    out = torch.arange(12, dtype=torch.float32).reshape(6, 2)
    assert R.vote_add_ref(votes, counts, ids, out) == 2
    assert votes.tolist() == [[0, 0], [10, 11], [0, 0], [2, 3]] and counts.tolist() == [0, 1, 0, 1]
