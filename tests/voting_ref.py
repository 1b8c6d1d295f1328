"""CPU restatements for the voting tests (TEST INFRASTRUCTURE ONLY): the arithmetic csrc/vote.hip implements, written
in torch / numpy float32, and the three tracker flows built from it as plain functions.

  * votes: ``votes[ids] += outputs; counts[ids] += 1`` where an id that occurs several times counts once, its LAST
    occurrence -- a sequential loop;
  * K-NN: ``oracle.knn_oracle.knn_bruteforce`` extended to query != search: the k smallest float32 squared distances
    ((dx^2 + dy^2) + dz^2), ascending by (d2, search index);
  * interpolation: w_r = 1 / max(d2_r, 1e-16); num = ((0 + x[nbr_0] w_0) + x[nbr_1] w_1) + ...; den likewise; y = num /
    den, a loop over the neighbour ranks with every operation rounded on its own;
  * the S3DIS, ScanNet / SegmentationVoter and KITTI-360 flows on top of these.
"""
import numpy as np
import torch


def vote_add_ref(votes, counts, ids, outputs):
    """In place on CPU tensors (votes float32 [N, C], counts int32 [N]); returns the number of ids outside [0, N)."""
    N = votes.shape[0]
    out = outputs.to(torch.float32)
    last, n_bad = {}, 0
    for p, i in enumerate(ids.tolist()):
        if 0 <= i < N:
            last[i] = p                                     # a later occurrence replaces an earlier one
        else:
            n_bad += 1
    for i, p in last.items():
        votes[i] = votes[i] + out[p]
        counts[i] = counts[i] + 1
    return n_bad


def knn_ref(query, search, k):
    """(neighbors int32 [n, k], dist2 float32 [n, k]) of every query among the search points."""
    q = np.asarray(query, dtype=np.float32)
    s = np.asarray(search, dtype=np.float32)
    n, m = q.shape[0], s.shape[0]
    assert k <= m
    nbr = np.empty((n, k), dtype=np.int32)
    d2o = np.empty((n, k), dtype=np.float32)
    idx = np.arange(m)
    for i in range(n):
        e = s - q[i][None, :]
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]          # fp32, left to right
        order = np.lexsort((idx, d2))[:k]
        nbr[i] = order
        d2o[i] = d2[order]
    return nbr, d2o


def interpolate_ref(x, nbr, d2):
    """y float32 [n, C] from x float32 [M, C] and the neighbour tables: the rank-order loop."""
    x = torch.as_tensor(x, dtype=torch.float32)
    nbr = torch.as_tensor(np.asarray(nbr)).long()
    d2 = torch.as_tensor(np.asarray(d2), dtype=torch.float32)
    n, k = nbr.shape
    num = torch.zeros((n, x.shape[1]), dtype=torch.float32)
    den = torch.zeros((n, 1), dtype=torch.float32)
    for r in range(k):
        w = 1.0 / torch.clamp(d2[:, r:r + 1], min=1e-16)
        num = num + x[nbr[:, r]] * w
        den = den + w
    return num / den


def interpolate_index_add_form(x, pos_x, pos_y, nbr):
    """The lines of torch_geometric's knn_interpolate after its K-NN: pairs (y_idx, x_idx) in query-major, rank-minor
    order, squared distances recomputed from the positions, two scatter-adds (index_add_ on the CPU adds in order)."""
    x = torch.as_tensor(x, dtype=torch.float32)
    pos_x = torch.as_tensor(pos_x, dtype=torch.float32)
    pos_y = torch.as_tensor(pos_y, dtype=torch.float32)
    nbr = torch.as_tensor(np.asarray(nbr)).long()
    n, k = nbr.shape
    y_idx = torch.arange(n).repeat_interleave(k)
    x_idx = nbr.reshape(-1)
    diff = pos_x[x_idx] - pos_y[y_idx]
    squared_distance = (diff * diff).sum(dim=-1, keepdim=True)
    weights = 1.0 / torch.clamp(squared_distance, min=1e-16)
    y = torch.zeros((n, x.shape[1]), dtype=torch.float32).index_add_(0, y_idx, x[x_idx] * weights)
    return y / torch.zeros((n, 1), dtype=torch.float32).index_add_(0, y_idx, weights)


def knn_interpolate_ref(x, pos_x, pos_y, k):
    nbr, d2 = knn_ref(pos_y, pos_x, k)
    return interpolate_ref(x, nbr, d2)


def argmax_first(y):
    """numpy's argmax: the first maximum, a NaN is the maximum."""
    return np.argmax(np.asarray(y), axis=1).astype(np.int64)


def confusion_ref(labels, pred, C, ignore=None):
    """(matrix int64 [C, C], n_bad): pairs whose label is ``ignore`` are skipped, other labels outside [0, C) counted
    in n_bad."""
    labels, pred = np.asarray(labels).astype(np.int64), np.asarray(pred).astype(np.int64)
    keep = np.ones(labels.shape, dtype=bool) if ignore is None else labels != ignore
    bad = keep & ((labels < 0) | (labels >= C))
    ok = keep & ~bad
    return np.bincount(labels[ok] * C + pred[ok], minlength=C * C).reshape(C, C).astype(np.int64), int(bad.sum())


def s3dis_flow(votes, counts, pos, y):
    """s3dis_tracker.py:70-78 (vote confusion over the voted points) and :94-118 (k = 1 interpolation of the vote
    sums to every point)."""
    C = votes.shape[1]
    has = counts > 0
    vote_cm, _ = confusion_ref(y[has].numpy(), argmax_first(votes[has]), C)
    full = knn_interpolate_ref(votes[has], pos[has], pos, 1)
    pred = argmax_first(full)
    full_cm, _ = confusion_ref(y.numpy(), pred, C)
    return {"vote_cm": vote_cm, "pred": pred, "full_cm": full_cm}


def voter_flow(votes, counts, pos, k, class_seg_map=None):
    """segmentation_helpers.py:52-57, 76-83: votes divided by their counts, interpolated, argmax (over the columns of
    class_seg_map, shifted by its first entry)."""
    has = counts > 0
    v = votes[has].div(counts[has].to(torch.float32).unsqueeze(-1))
    full = knn_interpolate_ref(v, pos[has], pos, k)
    if class_seg_map:
        return argmax_first(full[:, class_seg_map]) + class_seg_map[0]
    return argmax_first(full)


def kitti360_flow(votes, counts, pos, y, ignore):
    """kitti360_tracker.py:192-193, 205-209 (vote confusion without the ignored labels) and :219-232 (points with a vote
    keep their own argmax, the others take the k = 1 interpolation)."""
    C = votes.shape[1]
    has = counts > 0
    vote_cm, _ = confusion_ref(y[has].numpy(), argmax_first(votes[has]), C, ignore)
    pred = argmax_first(votes)
    if bool((~has).any()):
        pred[(~has).numpy()] = argmax_first(knn_interpolate_ref(votes[has], pos[has], pos[~has], 1))
    full_cm, _ = confusion_ref(y.numpy(), pred, C, ignore)
    return {"vote_cm": vote_cm, "pred": pred, "full_cm": full_cm}


def keep_fill_ref(x, pos_x, pos_y, keep_counts, k):
    """ops.knn_interpolate_labels with keep_counts: the queries with a positive count are, in order, the rows of x and
    keep their own argmax; the others are interpolated."""
    kept = np.asarray(keep_counts) > 0
    own = np.cumsum(kept) - 1
    pred = argmax_first(knn_interpolate_ref(x, pos_x, pos_y, k))
    pred[kept] = argmax_first(torch.as_tensor(x)[own[kept]])
    return pred
