"""K-NN of a query cloud in a search cloud (dva_knn_query), per-point PCA (dva_pointwise_pca) and the
PCAComputePointwise / EigenFeatures transforms (reference core/data_transform/features.py:307-587) on the device:
against a brute-force fp32 search written here, against ops.knn, against the reference's own fixtures
(tests/golden/pca_*.npz) and against a float64 restatement of batch_pca under the gates of
tests/test_pointwise_pca_host.py."""
import importlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden, t
from test_pointwise_pca_host import SCENES, check_pca_against_f64, f64_pca, search_cloud

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bruteforce(query, search, k):
    """argKmin(k) of ((dx*dx + dy*dy) + dz*dz) in fp32, ascending by (d2, search index)."""
    e = query[:, None, :] - search[None, :, :]
    d = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    d2, idx = torch.sort(d, dim=1, stable=True)
    return idx[:, :k].int(), d2[:, :k]


def cloud(name, n, gen):
    if name == "uniform":
        return torch.rand(n, 3, generator=gen) * torch.tensor([4.0, 4.0, 2.5])
    if name == "voxel_grid":      # voxel centres: masses of exactly tied distances
        c = torch.unique(torch.randint(0, 14, (4 * n, 3), generator=gen), dim=0)
        return (c[torch.randperm(c.shape[0], generator=gen)[:n]].float() + 0.5) * 0.05
    if name == "clustered":       # very uneven density + far outliers
        return torch.cat([torch.randn(n - 10, 3, generator=gen) * 0.02, torch.randn(10, 3, generator=gen) * 30])
    raise ValueError(name)


def queries(kind, search, gen):
    lo, hi = search.min(0).values, search.max(0).values
    if kind == "subset":          # points of the search cloud itself: zero distances, duplicates in the voxel grid
        return search[torch.randperm(search.shape[0], generator=gen)[:400]].clone()
    if kind == "disjoint":        # fresh points in the box
        return lo + torch.rand(400, 3, generator=gen) * (hi - lo)
    if kind == "outside":         # beyond the box on every side
        d = torch.randn(400, 3, generator=gen)
        d = d / d.abs().max(1, keepdim=True).values
        return (lo + hi) / 2 + d * (hi - lo) * (0.6 + torch.rand(400, 1, generator=gen) * 2)
    raise ValueError(kind)


@pytest.mark.parametrize("name", ["uniform", "voxel_grid", "clustered"])
@pytest.mark.parametrize("kind", ["subset", "disjoint", "outside"])
@pytest.mark.parametrize("k", [1, 8, 50, 128])
def test_knn_query_matches_bruteforce(name, kind, k):
    from deepviewagg_amd import ops
    gen = torch.Generator().manual_seed(k + 7)
    search = cloud(name, 1500, gen)
    query = queries(kind, search, gen)
    if name == "voxel_grid" and kind == "disjoint":       # lattice points between the centres: tied distances
        query = torch.randint(0, 15, (400, 3), generator=gen).float() * 0.05
    ref_n, ref_d = bruteforce(query, search, k)
    for cell in (None, 0.07, 5.0):
        nbr, d2 = ops.knn_query(query.to(DEV), search.to(DEV), k, cell=cell)
        assert nbr.dtype == torch.int32 and nbr.shape == (query.shape[0], k)
        assert torch.equal(d2.cpu(), ref_d), (name, kind, k, cell)          # bit-identical fp32 distances
        assert torch.equal(nbr.cpu(), ref_n), (name, kind, k, cell)         # and tie order


@pytest.mark.parametrize("name", ["uniform", "voxel_grid", "clustered"])
def test_knn_query_on_the_cloud_itself_equals_knn(name):
    from deepviewagg_amd import ops
    gen = torch.Generator().manual_seed(3)
    xyz = cloud(name, 2000, gen).to(DEV)
    for k in (8, 50):
        n1, d1 = ops.knn(xyz, k)
        n2, d2 = ops.knn_query(xyz, xyz, k)
        assert torch.equal(n1, n2) and torch.equal(d1, d2), (name, k)


def test_knn_query_sizes():
    from deepviewagg_amd import ops
    search = torch.rand(30, 3, device=DEV)
    nbr, d2 = ops.knn_query(torch.zeros(0, 3, device=DEV), search, 5)
    assert nbr.shape == (0, 5) and d2.shape == (0, 5)
    nbr, _ = ops.knn_query(torch.rand(3, 3, device=DEV), search, 30)     # every search point
    assert torch.equal(nbr.sort(1).values.cpu(), torch.arange(30, dtype=torch.int32).expand(3, 30))
    with pytest.raises(ValueError):
        ops.knn_query(torch.rand(3, 3, device=DEV), search, 31)
    with pytest.raises(ValueError):
        ops.knn_query(torch.rand(3, 3, device=DEV), search, 129)


@pytest.mark.parametrize("scene", SCENES)
def test_neighbors_equal_the_reference(scene):
    from deepviewagg_amd import ops
    g = load_golden(scene)
    nbr, _ = ops.knn_query(t(g["pos"], DEV), search_cloud(g).to(DEV), int(g["k"]))
    assert torch.equal(nbr.cpu(), t(g["neighbors"]))


@pytest.mark.parametrize("scene", SCENES)
def test_pointwise_pca_against_f64(scene):
    """dva_pointwise_pca on the reference's neighbourhoods under the gates the reference's own output meets."""
    from deepviewagg_amd import ops
    g = load_golden(scene)
    search, nbr = search_cloud(g), t(g["neighbors"])
    evals, evecs = ops.pointwise_pca(search.to(DEV), nbr.to(DEV))
    assert evals.shape == (nbr.shape[0], 3) and evecs.shape == (nbr.shape[0], 9)
    evals, evecs = evals.cpu(), evecs.cpu()
    check_pca_against_f64(evals, evecs, search, nbr, f"dva_pointwise_pca {scene}")
    # unit rows; sign convention: the largest-magnitude component of every eigenvector is positive
    ev = evecs.view(-1, 3, 3)
    torch.testing.assert_close(ev.norm(dim=2), torch.ones(ev.shape[:2]), rtol=0, atol=1e-6)
    big = ev.gather(2, ev.abs().argmax(2, keepdim=True))
    assert bool((big > 0).all())
    # all-equal neighbourhoods (pca_degen: 40 copies of one point): exactly 0 and the identity
    w, _ = f64_pca(search, nbr)
    flat = (w == 0).all(1)
    if scene == "pca_degen":
        assert int(flat.sum()) == 40
    assert bool((evals[flat] == 0).all()) and bool((evecs[flat] == torch.eye(3).flatten()).all())


def test_pointwise_pca_degenerate_rules():
    """NaN / inf coordinates: eigenvalues 1 and the identity (features.py:320-323); identical neighbours: 0, the
    identity and linearity 1, planarity 0, scattering 0; indices outside the cloud are refused."""
    from deepviewagg_amd import ops
    from deepviewagg_amd.core.data_transform.features import EigenFeatures
    search = torch.rand(12, 3)
    search[5, 1] = float("nan")
    search[6, 2] = float("inf")
    search[8:] = torch.tensor([0.5, -1.0, 2.0])          # four identical points
    nbr = torch.tensor([[0, 1, 2, 3],         # regular
                        [0, 1, 5, 3],         # NaN
                        [6, 1, 2, 3],         # inf
                        [8, 9, 10, 11],       # identical points
                        [4, 4, 4, 4],         # one point four times
                        [7, 0, 2, 3]], dtype=torch.int32)
    evals, evecs = ops.pointwise_pca(search.to(DEV), nbr.to(DEV))
    evals, evecs = evals.cpu(), evecs.cpu()
    eye = torch.eye(3).flatten()
    for r in (1, 2):
        assert torch.equal(evals[r], torch.ones(3)) and torch.equal(evecs[r], eye), r
    for r in (3, 4):
        assert torch.equal(evals[r], torch.zeros(3)) and torch.equal(evecs[r], eye), r
    for r in (0, 5):
        assert bool(torch.isfinite(evals[r]).all()) and not torch.equal(evecs[r], eye)
    d = EigenFeatures()(SimpleNamespace(eigenvalues=evals, eigenvectors=evecs))
    assert torch.equal(d.linearity[3:5], torch.ones(2))
    assert torch.equal(d.planarity[3:5], torch.zeros(2)) and torch.equal(d.scattering[3:5], torch.zeros(2))
    with pytest.raises(ValueError):
        ops.pointwise_pca(search.to(DEV), torch.tensor([[0, 1, 2, 12]], dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.pointwise_pca(search.to(DEV), torch.tensor([[0, -1, 2, 3]], dtype=torch.int32, device=DEV))


def test_pointwise_pca_large_k_and_many_points():
    """k = 128 (the LDS tile of the kernel at its largest) and more points than one launch's grid covers."""
    from deepviewagg_amd import ops
    gen = torch.Generator().manual_seed(11)
    search = torch.rand(4000, 3, generator=gen) * torch.tensor([3.0, 2.0, 0.05])
    for n, k in ((700, 128), (600_000, 9)):
        nbr = torch.randint(0, 4000, (n, k), generator=gen, dtype=torch.int32)
        evals, evecs = ops.pointwise_pca(search.to(DEV), nbr.to(DEV))
        sel = torch.randperm(n, generator=gen)[:2000]
        check_pca_against_f64(evals.cpu()[sel], evecs.cpu()[sel], search, nbr[sel], f"n={n} k={k}")


def test_transforms_match_reference_fixtures():
    """PCAComputePointwise -> EigenFeatures: CPU Data in, CPU attributes out; use_full_pos searches data.full_pos."""
    from deepviewagg_amd.core.data_transform.features import EigenFeatures, PCAComputePointwise
    for scene in SCENES:
        g = load_golden(scene)
        full = "full_pos" in g
        data = SimpleNamespace(pos=t(g["pos"]), full_pos=t(g["full_pos"]) if full else None)
        data = PCAComputePointwise(num_neighbors=int(g["k"]), use_full_pos=full, use_faiss=False)(data)
        assert data.eigenvalues.device.type == "cpu" and data.eigenvectors.dtype == torch.float32
        data = EigenFeatures(temperature=5)(data)
        check_pca_against_f64(data.eigenvalues, data.eigenvectors, search_cloud(g), t(g["neighbors"]), scene)
        ref = np.stack([g[f + "_t5"] for f in ("linearity", "planarity", "scattering")], 1)
        got = torch.stack([data.linearity, data.planarity, data.scattering], 1)
        torch.testing.assert_close(got, t(ref), rtol=0, atol=7e-4)      # both within 5e-4 of the f64 features
    pair = PCAComputePointwise(num_neighbors=16)([SimpleNamespace(pos=t(g["pos"])) for _ in range(2)])
    assert len(pair) == 2 and torch.equal(pair[0].eigenvalues, pair[1].eigenvalues)


def test_end_to_end_through_the_reference_names():
    """dropin.install(); PCAComputePointwise -> EigenFeatures -> MapImages looked up by the reference's dotted names,
    as a data config instantiates them: the mapping features carry the computed linearity / planarity / scattering
    and MapImages reads data.norm for the orientation column."""
    import sys
    from deepviewagg_amd import dropin
    from deepviewagg_amd.core.multimodal.image import SameSettingImageData
    for k in [k for k in sys.modules if k.startswith("torch_points3d")]:
        del sys.modules[k]
    try:
        dropin.install(patch_existing=False)
        feats = importlib.import_module("torch_points3d.core.data_transform.features")
        mm = importlib.import_module("torch_points3d.core.data_transform.multimodal.image")
        g = load_golden("mapping_build")
        n = g["xyz"].shape[0]
        data = SimpleNamespace(pos=t(g["xyz"]), mapping_index=torch.arange(n))
        data = feats.PCAComputePointwise(num_neighbors=50, use_faiss=False)(data)
        data = feats.EigenFeatures(norm=True, linearity=True, planarity=True, scattering=True)(data)
        for a in ("eigenvalues", "eigenvectors", "norm", "linearity", "planarity", "scattering"):
            assert getattr(data, a).device.type == "cpu", a
        nbr, _ = bruteforce(data.pos, data.pos, 50)
        check_pca_against_f64(data.eigenvalues, data.eigenvectors, data.pos, nbr, "mapping_build cloud")

        def build(d):
            cams = t(g["cams"])
            images = SameSettingImageData(path=np.array([f"i{i}" for i in range(len(cams))]), pos=cams,
                                          opk=torch.zeros(len(cams), 3), ref_size=tuple(int(v) for v in g["ref_size"]),
                                          proj_upscale=int(g["proj_upscale"]))
            tr = mm.MapImages(method="SplattingVisibility", r_max=10.0, r_min=0.2, voxel=0.05, k_swell=1.0,
                              d_swell=1000, exact=True)
            return tr(d, images)[1].mappings
        m = build(data)
        assert m.device.type == "cpu" and m.features.shape[1] == 6 and m.features.shape[0] > 0
        pt = torch.arange(n).repeat_interleave(m.pointers[1:] - m.pointers[:-1])
        for c, a in ((1, "linearity"), (2, "planarity"), (3, "scattering")):
            assert torch.equal(m.features[:, c], getattr(data, a)[pt]), a
        flipped = SimpleNamespace(**vars(data))
        flipped.norm = torch.tensor([[0.0, 0.0, 1.0]]).expand(n, 3).contiguous()
        assert not torch.equal(build(flipped).features[:, 4], m.features[:, 4])     # orientation follows data.norm
    finally:
        for k in [k for k in sys.modules if k.startswith("torch_points3d")]:
            del sys.modules[k]
