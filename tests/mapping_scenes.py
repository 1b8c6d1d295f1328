"""Scenes that steer the batched visibility build (``dva_visibility_batch``) onto each of its code paths, and the
predicates -- computed from the C oracle alone -- that say a scene really gets there.

The kernel constants below are those of deepviewagg_amd/csrc/mapping.hip (``constexpr int ZT = 32, ZT_BIG = 16,
ZT_BIGCAP = 4096, ZT_CHUNK = 2048``; ``bin_blocks`` capped at 4096; ``list_cap = 4 * n * B``; ``n_img = T <= 4096 ? 2 :
(T <= 8192 ? 1 : 0)``; the tiled path taken when ``img_w < 65536 && Hc < 65536``).  They are not exported: whoever changes
them there moves the shapes here.

numpy only: tests/test_mapping_scenes_host.py asserts the predicates without a GPU, tests/test_gpu_mapping_dispatch.py
asserts them again before it trusts a comparison.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

from conftest import load_golden
from oracle import mapping_oracle as M

ZT = 32                 # screen tile edge, pixels
ZT_BIG = 16             # a box over more tiles than this goes to the per-image large-box list
ZT_BIGCAP = 4096        # slots of the large-box list of one image
ZT_CHUNK = 2048         # survivors per block sweep of the bin kernels
BIN_GRID_CAP = 4096     # blocks of the bin kernels
LIST_PER_CANDIDATE = 4  # tile-list capacity: entries per candidate and image
N_IMG_2_MAX_T = 4096    # tiles per image up to which a block keeps the counters of two images in LDS
N_IMG_1_MAX_T = 8192    # ... of one image; beyond: global counters only
ATOMIC_PLANE_MIN_W = 65536   # image width (or cropped height) from which the batch takes the atomic plane
QUARTER_WAVE_MAX_AREA = 128  # zbuffer_batch_kernel: four boxes of at most this many pixels share a wavefront

@dataclass
class Scene:
    name: str
    camera: str
    kw: dict                      # SplattingVisibility / make_camera settings except ``exact``
    xyz: np.ndarray               # [n, 3] float32
    img_xyz: np.ndarray           # [B, 3] float32
    per_image: dict = field(default_factory=dict)   # img_opk [B, 3] | img_extrinsic [B, 4, 4] | intrinsics [B, ...]
    mask: np.ndarray = None       # [W, H] uint8, shared by the images
    attrs: dict = field(default_factory=dict)

    @property
    def B(self):
        return self.img_xyz.shape[0]

    @property
    def n(self):
        return self.xyz.shape[0]

    @property
    def Hc(self):
        return self.kw["img_size"][1] - self.kw["crop_top"] - self.kw["crop_bottom"]

    @property
    def tiles_per_image(self):
        return -(-self.kw["img_size"][0] // ZT) * -(-self.Hc // ZT)


def model_of(scene, exact):
    from deepviewagg_amd.core.multimodal.visibility import SplattingVisibility
    return SplattingVisibility(camera=scene.camera, exact=exact, **scene.kw)


def oracle_camera(scene, i, exact=False):
    kw = scene.kw
    return M.make_camera(scene.camera, kw["img_size"], scene.img_xyz[i], crop_top=kw["crop_top"],
                         crop_bottom=kw["crop_bottom"], r_min=kw["r_min"], r_max=kw["r_max"], voxel=kw["voxel"],
                         k_swell=kw["k_swell"], d_swell=kw["d_swell"], exact=exact,
                         **{k: v[i] for k, v in scene.per_image.items()})


def oracle_survivors(scene, i):
    """(idx, dist, x_proj, y_proj) of the candidates that survive camera i's projection, in candidate order."""
    return M.camera_projection(scene.xyz, oracle_camera(scene, i), scene.mask)


def oracle_boxes(scene, i):
    """[m, 4] (x0, x1, y0, y1) splat boxes of camera i's survivors, y in CROPPED coordinates like the kernels'."""
    idx, dist, xp, yp = oracle_survivors(scene, i)
    if len(idx) == 0:
        return np.zeros((0, 4), np.int64)
    box = M.splat(xp, yp, dist, scene.xyz[idx], oracle_camera(scene, i)).astype(np.int64)
    box[:, 2:] -= scene.kw["crop_top"]
    return box


def box_tiles(box):
    return ((box[:, 1] - 1) // ZT - box[:, 0] // ZT + 1) * ((box[:, 3] - 1) // ZT - box[:, 2] // ZT + 1)


def box_area(box):
    return (box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2])


def large_boxes(scene, i):
    """Boxes of image i that go to the large-box list."""
    return int((box_tiles(oracle_boxes(scene, i)) > ZT_BIG).sum())


def list_entries(scene, i):
    """Tile-list entries of image i: tiles summed over the boxes that do not go to the large-box list."""
    t = box_tiles(oracle_boxes(scene, i))
    return int(t[t <= ZT_BIG].sum())


def oracle_rows(scene, i, exact):
    return M.visibility(scene.xyz, oracle_camera(scene, i, exact), scene.mask)


@functools.lru_cache(maxsize=32)
def cached_oracle_rows(name, i, exact):
    """Oracle rows of a camera-model scene: shared by the tests of that scene, never modified."""
    return oracle_rows(camera_model_scene(name), i, exact)


def oracle_features(scene, i, rows, with_attrs):
    return M.mapping_features(scene.xyz, rows, oracle_camera(scene, i), **(scene.attrs if with_attrs else {}))


def room_cloud(n, rng, size=(8.0, 6.0, 3.0)):
    """Points on the six faces of a box room (the cloud of tests/test_gpu_mapping.py)."""
    face = rng.integers(0, 6, n)
    uvw = rng.random((n, 3))
    uvw[np.arange(n), face // 2] = face % 2
    return (uvw * np.array(size) + np.clip(rng.normal(0, 1e-3, (n, 3)), -0.05, 0.05)).astype(np.float32)


def point_attributes(n, rng):
    nrm = rng.normal(0, 1, (n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return dict(linearity=rng.random(n).astype(np.float32), planarity=rng.random(n).astype(np.float32),
                scattering=rng.random(n).astype(np.float32), normals=nrm.astype(np.float32))


def shell(center, n, r0, r1, rng):
    u = rng.normal(0, 1, (n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (np.asarray(center, np.float64) + u * rng.uniform(r0, r1, (n, 1))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# 1. camera models at scale: scannet, kitti360_perspective, kitti360_fisheye
# ---------------------------------------------------------------------------------------------------------------
# Per camera: the fixture, crops, a masked fraction, the focal length that sizes a box (pixels per unit of tangent; the
# fisheye's is its value at the image centre, gamma / (1 + xi)), the principal point, and for each layer of the cloud
# (count, distance range from camera 0 in metres, window of the view in fractions of the image: s0, s1, t0, t1).
# The near cluster (0.25 m .. 0.9 m) sits in the left part of the view: its boxes are hundreds of pixels wide, and spread
# over the whole view they would hide everything else (a handful of rows in exact mode).  The middle shell is placed
# where its boxes span 3 .. 4 tiles per axis (9 .. 16 list entries each).  The background is a slanted surface (depth
# grows with the image column), so that most of its points keep a visible edge.
CAMERA_MODELS = {
    "scannet": dict(
        golden="vis_pinhole_scannet", img_size=(320, 240), crop=(0, 0), masked=0.0,
        near=(14000, 0.25, 0.9, (0.02, 0.22, 0.30, 0.70)), mid=(22000, 0.80, 1.15, (0.0, 0.45, 0.0, 1.0)),
        back=(20000, 4.0, 7.5, (0.0, 1.0, 0.0, 1.0)), yaw=(0.0, -0.10, 0.08, 0.15), shift=0.03),
    "kitti360_perspective": dict(
        golden="vis_pinhole_kitti", img_size=(1408, 376), crop=(30, 21), masked=0.2,
        near=(8000, 0.25, 0.9, (0.05, 0.25, 0.30, 0.70)), mid=(30000, 1.45, 2.1, (0.0, 0.55, 0.0, 1.0)),
        back=(18000, 6.0, 15.0, (0.0, 1.0, 0.0, 1.0)), yaw=(0.0, -0.15, 0.10, -0.25), shift=0.03),
    "kitti360_fisheye": dict(
        golden="vis_fisheye_kitti", img_size=(1400, 1400), crop=(0, 0), masked=0.0,
        near=(6000, 0.25, 0.9, (0.25, 0.40, 0.35, 0.65)), mid=(33000, 1.45, 2.1, (0.2, 0.6, 0.2, 0.8)),
        back=(17000, 6.0, 15.0, (0.0, 1.0, 0.0, 1.0)), yaw=(0.0, -0.15, 0.10, -0.25), shift=0.03),
}


def _yaw4(theta):
    """Rotation about the camera's vertical (y) axis, homogeneous, float32."""
    c, s = np.float32(np.cos(theta)), np.float32(np.sin(theta))
    return np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def camera_model_scene(camera):
    spec = CAMERA_MODELS[camera]
    g = load_golden(spec["golden"])
    rng = np.random.default_rng(sorted(CAMERA_MODELS).index(camera) + 100)
    W, H = spec["img_size"]
    ext0 = g["img_extrinsic"].astype(np.float32)
    if "img_intrinsic_pinhole" in g:
        k = g["img_intrinsic_pinhole"]
        f, cx, cy = float(k[0, 0]), float(k[0, 2]), float(k[1, 2])
    else:
        fe = g["img_intrinsic_fisheye"]
        f, cx, cy = float(fe[3] / (1.0 + fe[0])), float(fe[5]), float(fe[6])

    def layer(count, d0, d1, window, slanted=False):
        s = rng.uniform(window[0], window[1], count)
        t = rng.uniform(window[2], window[3], count)
        ray = np.stack([(s * W - cx) / f, (t * H - cy) / f, np.ones(count)], 1)
        ray /= np.linalg.norm(ray, axis=1, keepdims=True)
        if slanted:
            d = d0 + (d1 - d0) * (s - window[0]) / (window[1] - window[0]) + rng.normal(0, 2e-3, count)
        else:
            d = rng.uniform(d0, d1, count)
        cam_frame = ray * d[:, None]
        return cam_frame @ ext0[:3, :3].astype(np.float64).T + ext0[:3, 3].astype(np.float64)

    xyz = np.concatenate([layer(*spec["near"]), layer(*spec["mid"]), layer(*spec["back"], slanted=True)])
    xyz = xyz[rng.permutation(len(xyz))].astype(np.float32)
    B = len(spec["yaw"])
    ext = np.stack([ext0 @ _yaw4(th) for th in spec["yaw"]]).astype(np.float32)
    move = rng.normal(0, spec["shift"], (B, 3)).astype(np.float32)
    move[0] = 0
    ext[:, :3, 3] = ext0[:3, 3] + move
    ext[0] = ext0
    per_image = dict(img_extrinsic=ext)
    for key in ("img_intrinsic_pinhole", "img_intrinsic_fisheye"):
        if key in g:
            per_image[key] = np.repeat(g[key][None].astype(np.float32), B, 0)
    mask = None
    if spec["masked"] > 0:
        mask = (rng.random((W, H)) >= spec["masked"]).astype(np.uint8)
    kw = dict(img_size=(W, H), crop_top=spec["crop"][0], crop_bottom=spec["crop"][1], r_min=float(g["r_min"]),
              r_max=float(g["r_max"]), voxel=0.15, k_swell=1.0, d_swell=1000)
    return Scene(camera, camera, kw, xyz, ext[:, :3, 3].copy(), per_image, mask, point_attributes(len(xyz), rng))


# ---------------------------------------------------------------------------------------------------------------
# equirectangular scenes
# ---------------------------------------------------------------------------------------------------------------
ROOM_CAMS = np.array([[3.1, 2.2, 1.4], [5.0, 3.0, 1.2], [2.0, 4.5, 1.6], [6.5, 1.5, 1.5], [4.0, 3.0, 2.0]], dtype=np.float32)


def _equirect_kw(img_size, r_min, r_max, voxel):
    return dict(img_size=tuple(img_size), crop_top=0, crop_bottom=0, r_min=r_min, r_max=r_max, voxel=voxel, k_swell=1.0,
                d_swell=1000)


# 2. tile-counter placement: (image size) -> (tiles per image, images of counters a block keeps in LDS)
COUNTER_SIZES = {(4096, 1024): (4096, 2), (4096, 1056): (4224, 1), (4096, 2048): (8192, 1), (4096, 2080): (8320, 0)}


def size_id(img_size):
    return f"{img_size[0]}x{img_size[1]}"


def counters_in_lds(T):
    return 2 if T <= N_IMG_2_MAX_T else (1 if T <= N_IMG_1_MAX_T else 0)


@functools.lru_cache(maxsize=2)
def tile_counter_scene(img_size, n, B):
    rng = np.random.default_rng(11)
    xyz = room_cloud(n, rng)
    opk = rng.normal(0, 0.3, (B, 3)).astype(np.float32)
    return Scene(f"counters{img_size[0]}x{img_size[1]}n{n}", "s3dis_equirectangular",
                 _equirect_kw(img_size, 0.05, 8.0, 0.02), xyz, ROOM_CAMS[:B].copy(), dict(img_opk=opk))


# 3. second sweep of the bin kernels: more survivors than BIN_GRID_CAP * ZT_CHUNK
@functools.lru_cache(maxsize=1)
def second_sweep_scene():
    rng = np.random.default_rng(12)
    B = 32
    xyz = room_cloud(270_000, rng)
    cams = (np.array([1.0, 1.0, 0.5]) + rng.random((B, 3)) * np.array([6.0, 4.0, 2.0])).astype(np.float32)
    opk = rng.normal(0, 0.3, (B, 3)).astype(np.float32)
    return Scene("second_sweep", "s3dis_equirectangular", _equirect_kw((256, 128), 0.05, 20.0, 0.02), xyz, cams,
                 dict(img_opk=opk))


# 4. atomic-plane batch path (W = 65536) and the 16-bit box packing at its limit (W = 65535)
WIDE_FAR, WIDE_NEAR = 8000, 6000


@functools.lru_cache(maxsize=2)
def wide_scene(width):
    """The cloud is NOT shuffled: a run of far points (small boxes: whole groups of four consecutive survivors take the
    quarter-wavefront sweep of zbuffer_batch_kernel), a run of near points (boxes beyond 128 pixels: the whole-wavefront
    sweep), then a mixture of both."""
    rng = np.random.default_rng(13)
    cams = (ROOM_CAMS[0] + np.array([[0, 0, 0], [0.06, -0.04, 0.03], [-0.05, 0.05, -0.04]])).astype(np.float32)
    far = shell(cams[0], WIDE_FAR, 3.0, 8.0, rng)
    near = shell(cams[0], WIDE_NEAR, 0.15, 0.28, rng)
    mixed = np.concatenate([shell(cams[0], 3000, 3.0, 8.0, rng), shell(cams[0], 3000, 0.15, 0.28, rng)])
    xyz = np.concatenate([far, near, mixed[rng.permutation(len(mixed))]]).astype(np.float32)
    opk = rng.normal(0, 0.3, (3, 3)).astype(np.float32)
    return Scene(f"wide{width}", "s3dis_equirectangular", _equirect_kw((width, 32), 0.05, 10.0, 0.005), xyz, cams,
                 dict(img_opk=opk))


# 5. empty images inside a batch
FAR_AWAY = 100.0     # metres: beyond r_max from every point of the scene


@functools.lru_cache(maxsize=None)
def empty_images_scene(camera, seeing):
    """B = 5; only the cameras ``seeing`` see the scene, the others stand FAR_AWAY from it."""
    seeing = tuple(seeing)
    rng = np.random.default_rng(14)
    B = 5
    if camera == "s3dis_equirectangular":
        xyz = room_cloud(20_000, rng)
        cams = ROOM_CAMS[:B].copy()
        cams[[b for b in range(B) if b not in seeing]] += np.float32(FAR_AWAY)
        opk = rng.normal(0, 0.3, (B, 3)).astype(np.float32)
        scene = Scene(f"empty_equirect{seeing}", camera, _equirect_kw((512, 256), 0.05, 8.0, 0.02), xyz, cams,
                      dict(img_opk=opk))
    else:
        base = camera_model_scene("scannet")
        keep = np.sort(rng.permutation(base.n)[:20_000])
        ext = np.repeat(base.per_image["img_extrinsic"][:1], B, 0).copy()
        ext[:, :3, 3] += rng.normal(0, 0.03, (B, 3)).astype(np.float32)
        for b in range(B):
            if b not in seeing:
                ext[b, :3, 3] += np.float32(FAR_AWAY)
        per_image = dict(img_extrinsic=ext,
                         img_intrinsic_pinhole=np.repeat(base.per_image["img_intrinsic_pinhole"][:1], B, 0))
        kw = dict(base.kw, voxel=0.03)
        scene = Scene(f"empty_scannet{seeing}", camera, kw, base.xyz[keep], ext[:, :3, 3].copy(), per_image)
    scene.attrs = point_attributes(scene.n, rng)
    return scene


# ---------------------------------------------------------------------------------------------------------------
# preconditions: asserted by the host test, and again by the GPU test before it compares anything
# ---------------------------------------------------------------------------------------------------------------
MIN_ROWS = 1000


def check_camera_model_scene(camera):
    sc = camera_model_scene(camera)
    assert 50_000 <= sc.n <= 60_000 and sc.B == 4
    # (a) one more large box than the large-box list of image 0 holds -- at the least
    assert large_boxes(sc, 0) > ZT_BIGCAP, large_boxes(sc, 0)
    # (b) a batch of one on image 0 overflows its tile lists with boxes that do not go to the large-box list
    assert list_entries(sc, 0) > LIST_PER_CANDIDATE * sc.n, (list_entries(sc, 0), LIST_PER_CANDIDATE * sc.n)
    # (c) every image keeps enough rows in exact mode for the comparison to say something
    for i in range(sc.B):
        assert len(cached_oracle_rows(camera, i, True)["idx"]) >= MIN_ROWS, i
    # the near cluster stands 0.25 m .. 0.9 m from camera 0
    d = np.linalg.norm(sc.xyz.astype(np.float64) - sc.img_xyz[0], axis=1)
    assert int(((d > 0.249) & (d < 0.901)).sum()) >= CAMERA_MODELS[camera]["near"][0]
    if camera == "kitti360_perspective":
        assert sc.Hc == 325 and sc.Hc % ZT != 0
        assert sc.mask.shape == (1408, 376) and 0.18 < 1.0 - sc.mask.mean() < 0.22
        # the mask culls survivors in the rows that only the uncropped height indexes right
        unmasked = M.camera_projection(sc.xyz, oracle_camera(sc, 0), None)[0]
        assert len(oracle_survivors(sc, 0)[0]) < 0.85 * len(unmasked)
    return sc


def check_tile_counter_scene(img_size, n, B):
    sc = tile_counter_scene(img_size, n, B)
    T, n_img = COUNTER_SIZES[img_size]
    assert sc.tiles_per_image == T and counters_in_lds(T) == n_img
    if img_size in ((4096, 1024), (4096, 2048)):
        assert 2 * n_img * T * 4 == 65536         # the fill pass asks for exactly 64 KiB of dynamic LDS
    for i in range(B):
        assert len(oracle_survivors(sc, i)[0]) == n     # image-major survivors: a chunk of ZT_CHUNK crosses images
    if n < ZT_CHUNK:
        assert n_img < 2          # a chunk of survivors reaches an image whose counters the block does not hold in LDS
    return sc


def check_second_sweep_scene():
    sc = second_sweep_scene()
    total = sum(len(oracle_survivors(sc, i)[0]) for i in range(sc.B))
    assert total > BIN_GRID_CAP * ZT_CHUNK == 8_388_608, total
    assert sc.n * sc.B * ZT_BIG <= 0x7fffffff          # still the tiled path
    return sc


def check_wide_scene(width):
    sc = wide_scene(width)
    assert (width >= ATOMIC_PLANE_MIN_W) == (width == 65536)
    for i in range(sc.B):
        idx = oracle_survivors(sc, i)[0]
        area = box_area(oracle_boxes(sc, i))
        assert int((area <= QUARTER_WAVE_MAX_AREA).sum()) >= MIN_ROWS and int((area > QUARTER_WAVE_MAX_AREA).sum()) >= MIN_ROWS
        # the far run survives whole and in place: its groups of four consecutive survivors are all small
        assert np.array_equal(idx[:WIDE_FAR], np.arange(WIDE_FAR))
        small = area[:WIDE_FAR] <= QUARTER_WAVE_MAX_AREA
        groups = small[:WIDE_FAR // 4 * 4].reshape(-1, 4).all(1)
        assert int(groups.sum()) >= 1000, int(groups.sum())
        assert WIDE_FAR >= 4000
        in_near_run = (idx >= WIDE_FAR) & (idx < WIDE_FAR + WIDE_NEAR)
        assert int(in_near_run.sum()) == WIDE_NEAR and (area[in_near_run] > QUARTER_WAVE_MAX_AREA).all()
    if width == 65535:
        assert any(int(oracle_boxes(sc, i)[:, 1].max()) == 65535 for i in range(sc.B))
    return sc


def check_empty_images_scene(camera, seeing):
    sc = empty_images_scene(camera, seeing)
    for i in range(sc.B):
        m = len(oracle_survivors(sc, i)[0])
        if i in seeing:
            assert m >= MIN_ROWS, (i, m)
        else:
            d = np.linalg.norm(sc.xyz.astype(np.float64) - sc.img_xyz[i], axis=1)
            assert d.min() > sc.kw["r_max"] and m == 0
    return sc
