"""Device voting and K-NN interpolation (csrc/vote.hip, ops.vote_add / knn_interpolate / knn_interpolate_labels,
metrics.full_res.VoteAccumulator, metrics.segmentation_helpers.SegmentationVoter) against the CPU restatements of
tests/voting_ref.py.  Every float comparison is bit for bit (torch.equal): the order of the arithmetic is fixed, votes
lie in [0, 64] and coordinates in [0, 1], so no subnormal takes part.  Shapes: around one wavefront (63, 64, 65), around
one block (257) and across blocks (1025)."""
import functools

import numpy as np
import pytest
import torch

import voting_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 300


@pytest.fixture(scope="module")
def ops():
    from deepviewagg_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------
# vote_add
# ---------------------------------------------------------------------------------------------

class _Votes:
    """The device accumulator and its CPU twin."""

    def __init__(self, ops, C, n=N):
        self.ops = ops
        self.votes, self.counts = torch.zeros(n, C, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
        self.slots = ops.vote_slots(n, DEV)
        self.ref_votes, self.ref_counts = torch.zeros(n, C), torch.zeros(n, dtype=torch.int32)

    def add(self, ids, out):
        n_bad = self.ops.vote_add(self.votes, self.counts, ids.to(DEV), out.to(DEV), self.slots)
        assert bool((self.slots == -1).all()), "the slot array reads all -1 after every call"
        ref_bad = R.vote_add_ref(self.ref_votes, self.ref_counts, ids, out)
        assert int(n_bad.item()) == ref_bad
        return ref_bad

    def check(self):
        assert torch.equal(self.votes.cpu(), self.ref_votes)
        assert torch.equal(self.counts.cpu(), self.ref_counts)


@pytest.mark.parametrize("C", [1, 13, 20, 64])
@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 257, 1025])
def test_vote_add_grid(ops, C, P):
    """P <= N: duplicate-free ids against torch's own ``votes[ids] += out`` on the CPU, two calls in a row (the counts
    reach 2).  P = 1025 exceeds the N = 300 points, so no duplicate-free ids exist: random ids, with duplicates, against
    the last-occurrence loop.  Every P also takes the random-ids case."""
    g = torch.Generator().manual_seed(100 * C + P)
    if P <= N:
        acc = _Votes(ops, C)
        tv, tc = torch.zeros(N, C), torch.zeros(N, dtype=torch.int32)
        ids = torch.randperm(N, generator=g)[:P]
        for _ in range(2):
            out = torch.rand(P, C, generator=g) * 8
            assert acc.add(ids, out) == 0
            tv[ids] += out
            tc[ids] += 1
        acc.check()
        assert torch.equal(acc.votes.cpu(), tv) and torch.equal(acc.counts.cpu(), tc)
        assert P == 0 or int(tc.max()) == 2
    acc = _Votes(ops, C)
    for _ in range(2):
        acc.add(torch.randint(0, N, (P,), generator=g), torch.rand(P, C, generator=g) * 8)
    acc.check()


@pytest.mark.parametrize("C", [1, 13, 64])
def test_vote_add_duplicates(ops, C):
    g = torch.Generator().manual_seed(7 + C)
    acc = _Votes(ops, C)
    acc.add(torch.arange(32).repeat_interleave(2), torch.rand(64, C, generator=g) * 8)       # twice in one wavefront
    acc.check()
    assert int(acc.counts.sum()) == 32
    out = torch.rand(1025, C, generator=g) * 8
    acc.add(torch.full((1025,), 17), out)                                                    # one id in every row
    acc.check()
    assert int(acc.counts[17]) == 2 and int(acc.counts.sum()) == 33
    acc.add(torch.arange(1025) % 256, torch.rand(1025, C, generator=g) * 8)                  # p, p + 256, ...: across blocks
    acc.check()
    acc.add(torch.arange(1025).flip(0) % 256, torch.rand(1025, C, generator=g) * 8)
    acc.check()


def test_vote_add_bad_ids_write_nothing(ops):
    g = torch.Generator().manual_seed(3)
    acc = _Votes(ops, 13)
    ids = torch.randperm(N, generator=g)[:65].clone()
    ids[[0, 31, 64]] = torch.tensor([-1, N, N + 5])
    assert acc.add(ids, torch.rand(65, 13, generator=g) * 8) == 3
    acc.check()
    assert int(acc.counts.sum()) == 62
    acc.add(torch.tensor([-1]), torch.rand(1, 13, generator=g))
    acc.check()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_vote_add_half_outputs_are_widened_exactly(ops, dtype):
    g = torch.Generator().manual_seed(5)
    acc = _Votes(ops, 20)
    for P in (65, 257):
        acc.add(torch.randint(0, N, (P,), generator=g), (torch.rand(P, 20, generator=g) * 8).to(dtype))
    acc.check()


def test_vote_add_is_reproducible(ops):
    g = torch.Generator().manual_seed(9)
    ids, out = torch.randint(0, N, (1025,), generator=g).to(DEV), (torch.rand(1025, 13, generator=g) * 8).to(DEV)
    runs = []
    for _ in range(2):
        votes, counts = torch.zeros(N, 13, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)
        ops.vote_add(votes, counts, ids, out, ops.vote_slots(N, DEV))
        runs.append((votes.cpu(), counts.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ---------------------------------------------------------------------------------------------
# knn_interpolate, knn_interpolate_labels
# ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _clouds(M, n, k):
    """Search cloud in [0.25, 0.75]^3 with duplicated points (the tie goes to the lower index); queries in [0, 1]^3, so
    some lie outside the search cloud's box, and every fourth one coincides with a search point (the 1e-16 clamp).  The
    K-NN restatement is computed once per (M, n, k) and shared by the cases of every C."""
    g = torch.Generator().manual_seed(1000 * M + 10 * n + k)
    pos_x = 0.25 + 0.5 * torch.rand(M, 3, generator=g)
    if M >= 4:
        pos_x[1] = pos_x[0]
        pos_x[M - 1] = pos_x[M // 2]
    pos_y = torch.rand(n, 3, generator=g)
    pos_y[::4] = pos_x[torch.randint(0, M, (len(range(0, n, 4)),), generator=g)]
    nbr, d2 = R.knn_ref(pos_y, pos_x, k)
    return pos_x, pos_y, nbr, d2


def _labels(n, C, g):
    labels = torch.randint(0, C, (n,), generator=g)
    labels[torch.rand(n, generator=g) < 0.1] = -1                    # 10 % ignored
    if n > 1:
        labels[n - 1] = C                                           # one label out of range
    return labels


@pytest.mark.parametrize("C", [1, 13, 20, 64])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("big", [False, True])
def test_knn_interpolate_grid(ops, big, n, k, C):
    M = 300 if big else k
    pos_x, pos_y, nbr, d2 = _clouds(M, n, k)
    g = torch.Generator().manual_seed(C)
    x = torch.rand(M, C, generator=g) * 64
    want = R.interpolate_ref(x, nbr, d2)
    xd, pxd, pyd = x.to(DEV), pos_x.to(DEV), pos_y.to(DEV)
    got_nbr, got_d2 = ops.knn_query(pyd, pxd, k)
    assert np.array_equal(got_nbr.cpu().numpy(), nbr) and np.array_equal(got_d2.cpu().numpy(), d2)
    y = ops.knn_interpolate(xd, pxd, pyd, k=k)
    assert torch.equal(y.cpu(), want)
    labels = _labels(n, C, g)
    pred, counts, n_bad = ops.knn_interpolate_labels(xd, pxd, pyd, k=k, labels=labels.to(DEV), num_classes=C,
                                                     ignore_index=-1)
    want_pred = R.argmax_first(want)
    assert np.array_equal(pred.cpu().numpy(), want_pred)
    want_counts, want_bad = R.confusion_ref(labels, want_pred, C, ignore=-1)
    assert np.array_equal(counts.cpu().numpy(), want_counts) and int(n_bad.item()) == want_bad == (1 if n > 1 else 0)
    only_pred, none_counts, none_bad = ops.knn_interpolate_labels(xd, pxd, pyd, k=k)
    assert torch.equal(only_pred, pred) and none_counts is None and none_bad is None
    if n == 257:                                                    # the result does not depend on the chunk
        assert torch.equal(ops.knn_interpolate(xd, pxd, pyd, k=k, chunk=64), y)
        out = torch.zeros(C, C, dtype=torch.int64, device=DEV)
        p2, c2, b2 = ops.knn_interpolate_labels(xd, pxd, pyd, k=k, labels=labels.to(DEV), num_classes=C, out=out,
                                                chunk=64)
        assert torch.equal(p2, pred) and c2 is out and torch.equal(c2, counts) and torch.equal(b2, n_bad)


def test_knn_interpolate_argmax_takes_the_first_maximum(ops):
    """Equal columns give equal interpolated values: the first one wins, also across the 16 lanes of a query."""
    pos_x, pos_y, nbr, d2 = _clouds(300, 65, 3)
    g = torch.Generator().manual_seed(2)
    x = torch.rand(300, 1, generator=g).mul(64).repeat(1, 64)
    x[:, :5] *= 0.5
    pred, _, _ = ops.knn_interpolate_labels(x.to(DEV), pos_x.to(DEV), pos_y.to(DEV), k=3)
    assert np.array_equal(pred.cpu().numpy(), R.argmax_first(R.interpolate_ref(x, nbr, d2)))
    assert bool((pred == 5).all())


@pytest.mark.parametrize("C", [1, 13, 20, 64])
@pytest.mark.parametrize("k", [1, 3])
def test_knn_interpolate_labels_keep_counts(ops, C, k):
    """KITTI-360's fill: the points with a vote keep their own argmax, also where a duplicated position would make
    another point their nearest neighbour."""
    g = torch.Generator().manual_seed(40 + C + k)
    n = 257
    pos = torch.rand(n, 3, generator=g)
    pos[1] = pos[0]
    keep = (torch.rand(n, generator=g) < 0.4).to(torch.int32) * torch.randint(1, 4, (n,), generator=g).to(torch.int32)
    keep[:2] = 1
    has = keep > 0
    x = torch.rand(int(has.sum()), C, generator=g) * 64
    want = R.keep_fill_ref(x, pos[has], pos, keep.numpy(), k)
    labels = _labels(n, C, g)
    pred, counts, n_bad = ops.knn_interpolate_labels(x.to(DEV), pos[has].to(DEV), pos.to(DEV), k=k,
                                                     labels=labels.to(DEV), keep_counts=keep.to(DEV), chunk=100)
    assert np.array_equal(pred.cpu().numpy(), want)
    want_counts, want_bad = R.confusion_ref(labels, want, C, ignore=-1)
    assert np.array_equal(counts.cpu().numpy(), want_counts) and int(n_bad.item()) == want_bad


def test_knn_interpolate_argument_errors(ops):
    x, pos_x, pos_y = torch.zeros(2, 3, device=DEV), torch.zeros(2, 3, device=DEV), torch.zeros(5, 3, device=DEV)
    with pytest.raises(ValueError, match="k = 3 neighbours requested from 2 points"):
        ops.knn_interpolate(x, pos_x, pos_y, k=3)
    with pytest.raises(ValueError, match="k = 3 neighbours requested from 2 points"):
        ops.knn_interpolate_labels(x, pos_x, pos_y, k=3)
    with pytest.raises(NotImplementedError):
        ops.knn_interpolate(x, pos_x, pos_y, batch_x=torch.zeros(2, dtype=torch.int64, device=DEV), k=1)
    assert tuple(ops.knn_interpolate(x, pos_x, pos_y[:0], k=1).shape) == (0, 3)


# ---------------------------------------------------------------------------------------------
# the three flows
# ---------------------------------------------------------------------------------------------

class _Data(dict):
    __getattr__ = dict.__getitem__


@functools.lru_cache(maxsize=None)
def _scene():
    """A raw cloud of 500 points, 13 classes, three overlapping samples of about 150 ids; the CPU votes are torch's own
    ``votes[ids] += out`` (the ids of one sample are distinct)."""
    g = torch.Generator().manual_seed(77)
    n, C = 500, 13
    pos = torch.rand(n, 3, generator=g)
    y = torch.randint(0, C, (n,), generator=g)
    samples = []
    for s in range(3):
        centre = torch.tensor([0.3 + 0.2 * s, 0.5, 0.5])
        ids = torch.argsort(((pos - centre) ** 2).sum(1))[:150]
        ids = ids[torch.randperm(150, generator=g)]
        samples.append((ids, torch.rand(150, C, generator=g) * 8))
    votes, counts = torch.zeros(n, C), torch.zeros(n, dtype=torch.int32)
    for ids, out in samples:
        votes[ids] += out
        counts[ids] += 1
    assert 0 < int((counts > 0).sum()) < n and int(counts.max()) >= 2
    return pos, y, samples, votes, counts


def _accumulate(samples):
    from deepviewagg_amd.metrics.full_res import VoteAccumulator
    acc = VoteAccumulator(500, 13, DEV)
    for ids, out in samples:
        acc.add(ids.to(DEV).reshape(-1, 1), out.to(DEV))            # [P, 1] ids, as a batched tracker sees them
    return acc


def _same_metrics(cm, host):
    from deepviewagg_amd.metrics.confusion_matrix import ConfusionMatrix
    assert np.array_equal(cm.confusion_matrix, host)
    assert cm.get_average_intersection_union() == ConfusionMatrix.create_from_matrix(host).get_average_intersection_union()


def test_s3dis_flow():
    pos, y, samples, votes, counts = _scene()
    want = R.s3dis_flow(votes, counts, pos, y)
    acc = _accumulate(samples)
    assert torch.equal(acc.votes.cpu(), votes) and torch.equal(acc.counts.cpu(), counts)
    assert torch.equal(acc.has_prediction.cpu(), counts > 0)
    assert acc.coverage == float(int((counts > 0).sum())) / 500
    _same_metrics(acc.vote_confusion(y.to(DEV)), want["vote_cm"])
    pred, cm = acc.full_res_predictions(pos.to(DEV), labels=y.to(DEV))
    assert np.array_equal(pred.cpu().numpy(), want["pred"])
    _same_metrics(cm, want["full_cm"])
    assert torch.equal(acc.full_res_predictions(pos.to(DEV)), pred)


@pytest.mark.parametrize("k", [1, 3])
def test_scannet_flow(k):
    pos, y, samples, votes, counts = _scene()
    want = R.voter_flow(votes, counts, pos, k)
    acc = _accumulate(samples)
    pred, cm = acc.full_res_predictions(pos.to(DEV), k=k, normalise=True, labels=y.to(DEV))
    assert np.array_equal(pred.cpu().numpy(), want)
    _same_metrics(cm, R.confusion_ref(y, want, 13)[0])


def test_kitti360_flow():
    pos, y, samples, votes, counts = _scene()
    y = y.clone()
    y[::7] = -1                                                     # ignored labels, voted and not
    want = R.kitti360_flow(votes, counts, pos, y, -1)
    acc = _accumulate(samples)
    _same_metrics(acc.vote_confusion(y.to(DEV), ignore_label=-1), want["vote_cm"])
    pred, cm = acc.full_res_predictions(pos.to(DEV), fill_only=True, labels=y.to(DEV), ignore_label=-1)
    assert np.array_equal(pred.cpu().numpy(), want["pred"])
    _same_metrics(cm, want["full_cm"])


@pytest.mark.parametrize("class_seg_map", [None, [4, 5, 6, 7]])
def test_segmentation_voter(class_seg_map):
    from deepviewagg_amd.core.data_transform.grid_transform import SaveOriginalPosId
    from deepviewagg_amd.metrics.segmentation_helpers import SegmentationVoter
    pos, y, samples, votes, counts = _scene()
    raw = _Data(pos=pos.to(DEV), y=y.to(DEV))
    voter = SegmentationVoter(raw, 13, "sparse", class_seg_map=class_seg_map, k=1)
    assert repr(voter) == "SegmentationVoter(num_pos=500)" and voter.num_votes == 0 and voter.coverage == 0.0
    voter.k = 3
    for ids, out in samples:                                        # one batch holding the sample after 20 other rows
        batch = _Data({SaveOriginalPosId.KEY: torch.cat([torch.zeros(20, dtype=torch.int64), ids]).to(DEV)})
        mask = torch.arange(170, device=DEV) >= 20
        voter.add_vote(batch, out.to(DEV), mask)
    assert voter.num_votes == 3 and voter.coverage == float(int((counts > 0).sum())) / 500
    assert voter.full_res_labels is raw.y
    want = R.voter_flow(votes, counts, pos, 3, class_seg_map)
    got = voter.full_res_preds
    assert got.dtype == torch.int64 and got.device.type == "cuda"
    assert np.array_equal(got.cpu().numpy(), want)


def test_no_prediction_is_a_value_error():
    from deepviewagg_amd.metrics.full_res import VoteAccumulator
    from deepviewagg_amd.metrics.segmentation_helpers import SegmentationVoter
    pos = torch.rand(50, 3, device=DEV)
    acc = VoteAccumulator(50, 13, DEV)
    with pytest.raises(ValueError, match="no point has a prediction"):
        acc.full_res_predictions(pos)
    with pytest.raises(ValueError, match="no point has a prediction"):
        SegmentationVoter(_Data(pos=pos, y=None), 13, "sparse").full_res_preds
    acc.add(torch.tensor([3, 50], device=DEV), torch.rand(2, 13, device=DEV))
    with pytest.raises(ValueError, match="1 origin ids lie outside"):
        acc.full_res_predictions(pos)
