"""CPU tests of PCAComputePointwise / EigenFeatures (reference core/data_transform/features.py:307-587) and of the
C-ABI entries behind them (dva_knn_query, dva_pointwise_pca): argument validation, the EigenFeatures expressions on
the reference's own fixture eigenvalues (tests/golden/pca_*.npz, tools/gen_golden_pointwise_pca.py), the accuracy
gates the GPU tests apply, constructors, and the drop-in alias.

The gates (``check_pca_against_f64``) compare a PCA with a float64 restatement of ``batch_pca`` on the same
neighbourhoods.  Each must pass for the reference's own fp32 output (``test_reference_output_passes_the_gates``):
  * eigenvalues: |l - l64| <= 2e-6 l_max (the reference: <= 8.5e-7 l_max on the fixtures);
  * eigenvectors, up to sign, where the eigenvalue is separated from the others by more than 1e-3 l_max:
    |v - v64| <= 1e-6 l_max / gap + 5e-7 (the reference: <= 3.7e-7 l_max / gap; 5e-7 absorbs the fp32 rounding of
    a unit vector);
  * EigenFeatures: |f - f64| <= 5e-4 (the reference: <= 2.1e-4).  The features take square roots of the
    eigenvalues, so the absolute error of an eigenvalue near 0 (a line, a plane) grows to its square root: the fp32
    reference's 3.7e-9 on a collinear neighbourhood of l_max 0.27 is a scattering error of 1.2e-4.
"""
import importlib
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, t

SCENES = ["pca_s3dis", "pca_kitti", "pca_voxel", "pca_degen"]
FEATURES = ("linearity", "planarity", "scattering")


def search_cloud(g):
    return t(g["full_pos"]) if "full_pos" in g else t(g["pos"])


def f64_pca(search, neighbors):
    """batch_pca (features.py:307-329) in float64: eigenvalues ascending clamped at 0, eigenvectors as rows."""
    x = search.double()[neighbors.long()]
    c = x - x.mean(dim=1, keepdim=True)
    w, v = torch.linalg.eigh(c.transpose(1, 2) @ c / x.shape[1])
    return w.clamp(min=0), v.transpose(1, 2)


def f64_features(w, temperature=None):
    r = w.sqrt()
    v0, v1, v2 = r[:, 0], r[:, 1], r[:, 2] + 1e-6
    f = torch.stack([(v2 - v1) / v2, (v1 - v0) / v2, v0 / v2], 1)
    if temperature:
        e = (temperature * f).exp()
        f = e / e.sum(dim=1, keepdim=True)
    return f


def check_pca_against_f64(evals, evecs, search, neighbors, what):
    """The accuracy gates of the module docstring; evals [n, 3], evecs [n, 9] (CPU tensors)."""
    from deepviewagg_amd.core.data_transform.features import EigenFeatures
    w, V = f64_pca(search, neighbors)
    lmax = w[:, 2:3]
    ew = evals.double()
    assert ew.shape == w.shape and bool((ew[:, 1:] >= ew[:, :-1]).all()) and bool((ew >= 0).all()), what
    err_w = (ew - w).abs()
    assert bool((err_w <= 2e-6 * lmax).all()), (what, float((err_w / lmax.clamp(min=1e-30)).max()))
    ev = evecs.double().view(-1, 3, 3)
    sign = torch.where((ev * V).sum(2, keepdim=True) < 0, -1.0, 1.0)
    err_v = (ev - sign * V).norm(dim=2)
    gap = torch.stack([torch.minimum((w[:, i] - w[:, j]).abs(), (w[:, i] - w[:, m]).abs())
                       for i, j, m in ((0, 1, 2), (1, 0, 2), (2, 0, 1))], 1)
    sep = gap > 1e-3 * lmax
    assert float(sep.double().mean()) > 0.5, what                  # the gate is not vacuous
    bound = 1e-6 * lmax.expand_as(gap) / gap.clamp(min=1e-300) + 5e-7
    bad = sep & (err_v > bound)
    assert not bool(bad.any()), (what, int(bad.sum()), float(err_v[sep].max()))
    for temperature in (None, 5):
        class D:
            eigenvalues, eigenvectors = evals, evecs
        d = EigenFeatures(temperature=temperature)(D)
        got = torch.stack([getattr(d, f) for f in FEATURES], 1).double()
        err_f = (got - f64_features(w, temperature)).abs().max()
        assert float(err_f) <= 5e-4, (what, temperature, float(err_f))


# ---------------------------------------------------------------------------------------------------------------
def test_argument_validation_of_the_new_entries_without_gpu():
    """Bad arguments are rejected with error codes before any HIP call."""
    from deepviewagg_amd import _lib
    lib = _lib.load()
    p = 16       # any non-null pointer value: validation fails before anything is dereferenced or launched
    wsb = lib.dva_knn_query_workspace_bytes
    assert wsb(-1, 10) == -1 and wsb(10, -1) == -1
    assert wsb(1 << 31, 10) == -2 and wsb(10, 1 << 31) == -2
    assert wsb(0, 10) > 0 and wsb(100, 1000) > wsb(0, 1000)

    def knn_query(qxyz=p, nq=10, sxyz=p, ns=100, bbox=p, cell=0.1, k=8, shells=2, nbr=p, ws=p, wsbytes=1 << 20):
        return lib.dva_knn_query(qxyz, nq, sxyz, ns, bbox, cell, k, shells, None, nbr, None, ws, wsbytes, None)
    assert knn_query(qxyz=None) == -1 and knn_query(sxyz=None) == -1 and knn_query(bbox=None) == -1
    assert knn_query(nbr=None) == -1 and knn_query(ws=None) == -1
    assert knn_query(k=0) == -1 and knn_query(k=129) == -1
    assert knn_query(ns=7) == -1                                   # n_search < k
    assert knn_query(nq=-1) == -1 and knn_query(cell=0.0) == -1 and knn_query(shells=0) == -1
    assert knn_query(nq=1 << 31) == -2 and knn_query(ns=1 << 31) == -2
    assert knn_query(nq=0, qxyz=None, nbr=None) == 0               # nothing to do

    def pca(sxyz=p, ns=100, nbr=p, nq=10, k=8, evals=p, evecs=p):
        return lib.dva_pointwise_pca(sxyz, ns, nbr, nq, k, evals, evecs, None)
    assert pca(sxyz=None) == -1 and pca(nbr=None) == -1 and pca(evals=None) == -1 and pca(evecs=None) == -1
    assert pca(k=0) == -1 and pca(k=129) == -1 and pca(ns=7) == -1 and pca(nq=-1) == -1
    assert pca(nq=1 << 31) == -2 and pca(ns=1 << 31) == -2
    assert pca(nq=0, nbr=None) == 0


def test_ops_refuse_cpu_tensors():
    from deepviewagg_amd import _lib, ops
    xyz = torch.rand(20, 3)
    with pytest.raises(_lib.DvaError):
        ops.knn_query(xyz, xyz, 4)
    with pytest.raises(_lib.DvaError):
        ops.pointwise_pca(xyz, torch.zeros(20, 4, dtype=torch.int32))


@pytest.mark.parametrize("scene", SCENES)
def test_eigen_features_equal_the_reference_on_its_eigenvalues(scene):
    """Same expressions on the same inputs: bit for bit, with and without temperature."""
    from deepviewagg_amd.core.data_transform.features import EigenFeatures
    g = load_golden(scene)
    for temperature, tag in ((None, ""), (5, "_t5")):
        class D:
            eigenvalues, eigenvectors = t(g["eigenvalues"]), t(g["eigenvectors"])
        d = EigenFeatures(temperature=temperature)(D)
        for f in ("norm",) + FEATURES:
            assert torch.equal(getattr(d, f), t(g[f + tag])), (scene, temperature, f)


def test_eigen_features_flags_and_lists():
    from deepviewagg_amd.core.data_transform.features import EigenFeatures
    g = load_golden("pca_s3dis")

    class D:
        def __init__(self):
            self.eigenvalues, self.eigenvectors = t(g["eigenvalues"]), t(g["eigenvectors"])
    out = EigenFeatures(norm=False, planarity=False)([D(), D()])
    assert len(out) == 2
    for d in out:
        assert not hasattr(d, "norm") and not hasattr(d, "planarity")
        assert torch.equal(d.linearity, t(g["linearity"])) and torch.equal(d.scattering, t(g["scattering"]))


@pytest.mark.parametrize("scene", SCENES)
def test_reference_output_passes_the_gates(scene):
    """The gates the GPU tests apply to dva_pointwise_pca are met by the reference's own fp32 batch_pca."""
    g = load_golden(scene)
    check_pca_against_f64(t(g["eigenvalues"]), t(g["eigenvectors"]), search_cloud(g), t(g["neighbors"]),
                          f"reference {scene}")


def test_constructors_repr_and_radius_error():
    from deepviewagg_amd.core.data_transform.features import EigenFeatures, PCAComputePointwise
    tr = PCAComputePointwise(num_neighbors=50, use_full_pos=True, use_faiss=False, chunk_size=10)
    assert (tr.num_neighbors, tr.r, tr.use_full_pos, tr.chunk_size) == (50, None, True, 10)
    cuda = torch.cuda.is_available()
    assert repr(tr) == (f"PCAComputePointwise(num_neighbors=50, r=None, use_full_pos=True, use_cuda=False, "
                        f"use_faiss=False, ncells=None, nprobes=10, chunk_size=10)")
    assert repr(PCAComputePointwise()) == (f"PCAComputePointwise(num_neighbors=40, r=None, use_full_pos=False, "
                                           f"use_cuda=False, use_faiss={cuda}, ncells=None, nprobes=10, "
                                           f"chunk_size=1000000)")
    assert repr(EigenFeatures(planarity=False, temperature=5)) == (
        "EigenFeatures(norm=True, linearity=True, planarity=False, scattering=True, temperature=5)")
    with pytest.raises(ValueError, match="radius"):
        PCAComputePointwise(num_neighbors=50, r=0.1)

    class NoFull:
        pos = torch.rand(10, 3)
    with pytest.raises(AssertionError, match="full_pos"):
        PCAComputePointwise(num_neighbors=4, use_full_pos=True)(NoFull)


def _drop_reference_modules():
    for k in [k for k in sys.modules if k.startswith("torch_points3d")]:
        del sys.modules[k]


def test_dropin_alias_resolves():
    from deepviewagg_amd import dropin
    from deepviewagg_amd.core.data_transform import features as ours
    _drop_reference_modules()
    try:
        assert "torch_points3d.core.data_transform.features" in dropin.install(patch_existing=False)
        ref = importlib.import_module("torch_points3d.core.data_transform.features")
        assert ref.PCAComputePointwise is ours.PCAComputePointwise and ref.EigenFeatures is ours.EigenFeatures
        # patched in place, a reference module keeps its other names: only the two classes are public here
        _drop_reference_modules()
        import types
        fake = types.ModuleType("torch_points3d.core.data_transform.features")
        fake.batch_pca = batch_pca = object()
        fake.PCACompute = pca_compute = object()
        sys.modules[fake.__name__] = fake
        dropin.install(patch_existing=True)
        assert fake.batch_pca is batch_pca and fake.PCACompute is pca_compute
        assert fake.PCAComputePointwise is ours.PCAComputePointwise and fake.EigenFeatures is ours.EigenFeatures
        assert [k for k in vars(ours) if not k.startswith("_")] == ["PCAComputePointwise", "EigenFeatures"]
    finally:
        _drop_reference_modules()
