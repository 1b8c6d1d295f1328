#!/usr/bin/env python
"""Headline benchmark of the DeepViewAgg multimodal hot path on MI355X.

metric (BASELINE.json): points/sec, fused forward+backward of
    multi-view gather -> atomic max-pool -> GroupBimodalCSRPool view attention -> concat fusion
on a synthetic 1M-point / 32-view scene per GPU (SURVEY.md §8(d) workload S1 / F-S):
    N = 2^20 points, 32 views each (V = 33.5 M), 32 feature maps [64 ch, 64x128] in bf16,
    8 mapping features per view, GroupBimodalCSRPool(in_map=8, in_mod=64, num_groups=4,
    map_encoder=DeepSetFeat, use_num=True) in TRAIN mode (batch-norm batch statistics).
The 2D encoder and the 3D backbone are outside the path.

    python bench.py --gpus N --steps K --warmup W
N > 1 is launched by the driver with torch.distributed.run (one rank per GPU, RCCL).  Every rank owns
its own scene (tile) -> weak scaling (--strong: one 2^20-point scene cut into N slabs); the collectives are the
all-reduce of the pooling module's parameter gradients and of a stand-in 112 MB fp32 bucket (--standin-mb: the rest of
the model's gradients), both on a side stream under the backward.  Rank 0 prints ONE compact JSON line
(< 4 KB, so that an 8 KB tail of stdout holds it): the contract fields + `roofline` (dominant kernel),
`roofline_view_gather_attention` (the fused kernel the north star names) and the top-8 kernels.  The full record (every
kernel, per-step arrays, notes) goes to `bench_detail.json` (`compact_line` / `emit`).

A plain run does only what that line needs: set-up, warm-up, the timed steps, --dump-outputs, the line.  --full adds
every other measurement after the timed steps (each still switched off by its --no-* option): the rocprofv3 PMC child
passes behind `roofline.traffic`, the HBM copy ceiling, the materialised gather + mapping build + K-NN (`gather`,
`mapping_build`, `neighborhood_features`), the secondary workloads (`workloads`) and `cpu_baseline` (C + OpenMP twin of
the whole step).
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec (6.3 TB/s measured copy)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log2-points", type=int, default=20)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also take every measurement beyond the headline: PMC traffic passes, "
                         "copy ceiling, gather / mapping build / K-NN, secondary workloads, CPU baselines (see the "
                         "--no-* options)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-log2-points", type=int, default=14)
    ap.add_argument("--no-mapping-build", action="store_true")
    ap.add_argument("--materialize", action="store_true",
                    help="diagnostic: materialised [V, C] gather + per-view E_mod (the reference's dataflow) instead "
                         "of the lazy gather / hoisted E_mod")
    ap.add_argument("--no-secondary", action="store_true", help="skip the S2 / F-L secondary workloads")
    ap.add_argument("--interpolate", action="store_true",
                    help="bilinear gather (interpolate=True, the published KITTI-360 configuration): mapping at 8x the "
                         "feature-map resolution, E_mod per view inside the chain kernels (fused_bilinear); with "
                         "--materialize: the reference's [V, C] dataflow")
    ap.add_argument("--out-channels", type=int, default=None,
                    help="out_mod of GroupBimodalCSRPool (default: --channels); the KITTI-360 pair is --channels 128 "
                         "--out-channels 32")
    ap.add_argument("--strong", action="store_true",
                    help="strong scaling: ONE scene of 2^log2-points points split into WORLD_SIZE spatial tiles "
                         "(parallel.tile_partition), each rank pools its tile (default: one scene per rank = weak)")
    ap.add_argument("--standin-mb", type=float, default=112.0,
                    help="N > 1: size (MB, fp32) of the stand-in gradient bucket for the parts of the model outside "
                         "the path (2D encoder + 3D backbone, SURVEY.md 8(e): 28.1 M parameters = 112 MB), "
                         "all-reduced on a side stream under the backward of every step; 0 disables")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help=argparse.SUPPRESS)   # gloo: only with --dry-run (the CPU test of the launcher)
    ap.add_argument("--dry-run", action="store_true",
                    help=argparse.SUPPRESS)   # launcher + process group + rank/device census only, no HIP work
    ap.add_argument("--no-standin", action="store_true", help="N > 1: no stand-in bucket (same as --standin-mb 0)")
    ap.add_argument("--no-pmc", action="store_true",
                    help="skip the two rocprofv3 --pmc child passes that measure roofline.traffic in this run (the "
                         "stamped file of the last evidence pass is used instead)")
    ap.add_argument("--detail-file", default=None,
                    help="where the full record goes (default: bench_detail.json in the repo root and in gpurun_out/)")
    ap.add_argument("--workload", default="S1", choices=["S1", "S2", "S1c"],
                    help="S1: every point seen by --views images (headline); S2: ragged view counts "
                         "min(views, 1 + Geom(0.2)), 10 %% of the points unseen (SURVEY.md 8(d))")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (rank 0) to DIR/<name>.npy in "
                         "float32, at most 64 MB in all: fused features, feature-map gradient (fixed seeded samples when "
                         "larger than 24 MB) and the view pooling module's parameter gradients (see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def make_scene(n_points, views, n_images, C, H, W, dtype, device, seed, workload="S1", upscale=1):
    """Synthetic scene of SURVEY.md §8(d).  S1: every point seen by `views` images at random pixels;
    S2: ragged view counts k_i = min(views, 1 + Geom(0.2)), 10 % of the points unseen.
    S1c (not in the survey; a locality probe): S1 with projection-like pixels -- the points lie on a raster in
    memory order and neighbouring points hit neighbouring pixels of every image (+-1 pixel jitter), as the
    points of a voxelised scan do; same number of views per feature-map row as S1."""
    g = torch.Generator(device=device).manual_seed(seed)
    if workload in ("S1", "S1c"):
        V = n_points * views
        csr = torch.arange(0, V + 1, views, dtype=torch.int64, device=device)
        # image ids: each point's views hit distinct images (sorted per point, like from_dense)
        if views == n_images:
            images = torch.arange(n_images, device=device).repeat(n_points)
        else:
            images = torch.stack([torch.randperm(n_images, generator=g, device=device)[:views].sort()[0]
                                  for _ in range(1024)]).repeat((n_points + 1023) // 1024, 1)[:n_points].reshape(-1)
    else:
        u = torch.rand(n_points, generator=g, device=device).clamp_(1e-9, 1 - 1e-9)
        k = (1 + torch.floor(torch.log(u) / float(torch.log(torch.tensor(0.8))))).long().clamp_(max=views)
        k[torch.rand(n_points, generator=g, device=device) < 0.1] = 0
        csr = torch.cat([torch.zeros(1, dtype=torch.int64, device=device), k.cumsum(0)])
        V = int(csr[-1])
        # k_i consecutive image ids from a random cyclic start, sorted inside the point
        start = torch.randint(0, n_images, (n_points,), generator=g, device=device).repeat_interleave(k)
        rank = torch.arange(V, device=device) - csr[:-1].repeat_interleave(k)
        pt = torch.arange(n_points, device=device).repeat_interleave(k)
        img = (start + rank) % n_images
        images = img[torch.argsort(pt * n_images + img)]
    if workload == "S1c":
        side = int(round(n_points ** 0.5))
        pid = torch.arange(n_points, device=device).repeat_interleave(views)
        u, v = pid % side, (pid // side).clamp_(max=side - 1)
        shift = torch.randint(0, 1 << 16, (n_images, 2), generator=g, device=device)[images]
        jit = torch.randint(-1, 2, (V, 2), generator=g, device=device)
        pixels = torch.stack([(u * W // side + shift[:, 0] + jit[:, 0]) % W,
                              (v * H // side + shift[:, 1] + jit[:, 1]) % H], 1).to(torch.int16)
    else:
        # upscale > 1 (bilinear workload): the mapping lives at upscale x the feature-map resolution
        pixels = torch.stack([torch.randint(0, W * upscale, (V,), generator=g, device=device),
                              torch.randint(0, H * upscale, (V,), generator=g, device=device)], 1).to(torch.int16)
    atom_ptr = torch.arange(V + 1, dtype=torch.int64, device=device)  # exact mapping: 1 pixel/view
    x = torch.randn(n_images, C, H, W, generator=g, device=device).to(dtype)
    x = x.contiguous(memory_format=torch.channels_last)
    x_map = torch.rand(V, 8, generator=g, device=device)
    x_3d = torch.randn(n_points, 4, generator=g, device=device)
    return dict(csr=csr, images=images.long(), pixels=pixels, atom_ptr=atom_ptr, x=x, x_map=x_map, x_3d=x_3d,
                mapping_size=(W * upscale, H * upscale))


def build_modules(C, device, C_out=None, pool="group"):
    from deepviewagg_amd.modules.multimodal.pooling import BimodalCSRPool, GroupBimodalCSRPool, QKVBimodalCSRPool
    from deepviewagg_amd.modules.multimodal.fusion import BimodalFusion
    torch.manual_seed(0)
    if pool == "qkv":
        # the reference's attentive pooling (modules/multimodal/pooling.py:454-547; late-fusion configs): queries from the
        # 3D features (x_3d [N, 4]), keys from the DeepSetFeat of the mapping features
        view_pool = QKVBimodalCSRPool(in_main=4, in_map=8, in_mod=C, num_groups=4, nc_qk=8, use_num=True).to(device).train()
    else:
        view_pool = GroupBimodalCSRPool(in_map=8, in_mod=C, out_mod=C_out, num_groups=4, use_mod=False,
                                        map_encoder='DeepSetFeat', use_num=True).to(device).train()
    return BimodalCSRPool(mode='max'), view_pool, BimodalFusion(mode='concatenation')


# HIP-event timer name -> kernel symbol in the rocprofv3 outputs (bf16 headline workload)
KERNEL_SYMBOL = {
    "chain_attn_fwd": "chain::attn_fwd_kernel<8, 4, 4>",
    "chain_attn_bwd": "chain::attn_bwd_kernel<unsigned short, 8, 4>",
    "chain_score_stats": "chain::score_stats_kernel",
    "chain_bwd_l6": "chain::layer_bwd_kernel<6, 3>",
    "chain_bwd_l5": "chain::layer_bwd_kernel<5, 3>",
    "chain_bwd_l2": "chain::layer_bwd_kernel<2, 3>",
    "chain_stats2": "chain::stats2_kernel",
    "chain_stats5": "chain::stats_mid_kernel<5>",
    "chain_stats6": "chain::stats_mid_kernel<6>",
    "chain_moments": "chain::moments_kernel",
    "view_gather_rows_grad": "ps::bucket_rows_grad_kernel<64, 8192>",
}
# what bounds the kernel the roofline object is about (SQ counters: profiles/*sq_counters*)
ROOFLINE_NOTES = {
    "view_gather_rows_grad": "rows gradient (deterministic, no atomics); since round 5 the 16-byte view records go through "
                             "pass A of the split plan (timer plan_sort_records) and ONE workgroup per bucket of 512 map rows "
                             "keeps the rows' sums in registers and consumes the bucket's records from LDS: per view 16 "
                             "streamed bytes and the 128-byte grad_out row of the point at a random address; bound by the "
                             "fabric's rate for one random line per view",
    "chain_bwd_l5": "layer-5 backward pass of the recompute chain (x_map 32 + index 4 + gradient row in 64 + out 64 bytes per "
                    "view, per-point rows): 166 VGPRs -> 3 wavefronts per SIMD; the one chain pass whose PMC traffic equals "
                    "its algorithmic bytes and whose vector unit is only ~0.5 busy: HBM-bound at 3 wavefronts per SIMD",
    "chain_attn_bwd": "attention backward from the stored scores (softmax / gate backward, score gradients, view "
                      "records; no chain evaluation): 107 VGPRs -> 4 wavefronts per SIMD; the value rows it re-gathers "
                      "(128 of its ~184 bytes per view) come out of the cache hierarchy",
    "*": "the recompute passes read 32-100 bytes per view by design (no stored activations): they are bound by VALU "
         "instruction issue, not by HBM or the matrix cores; their time, not their HBM fraction, is what is left to cut",
}
PMC_TRAFFIC_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "pmc_traffic_latest.json")


_LIVE_PMC = {"table": None, "why": "not run"}


def live_pmc_passes(timeout_s=150):
    """HBM traffic MEASURED IN THIS RUN: two child runs of this same script on the default workload
    (1 step after 1 warm-up, no secondary work) under `rocprofv3 --pmc FETCH_SIZE` and `--pmc WRITE_SIZE` -- separate passes
    with --kernel-trace only, as MI355X_MICROARCH.md's HBM section prescribes (the two counters do not fit one pass) --
    summarised by profiles/summarize_pmc.py (KiB units, FETCH_SIZE x 2 on gfx950, calibration on the copy kernel).  Fills
    _LIVE_PMC; on any failure (no rocprofv3, time-out, empty output) the stamped file of the last evidence pass stays
    the source and `why` says so."""
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        _LIVE_PMC["why"] = "rocprofv3 not found"
        return
    work = tempfile.mkdtemp(prefix="dva_pmc_", dir="/tmp")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["TMPDIR"] = "/tmp"
    # --full for the copy ceiling: its kernel is the calibration of summarize_pmc
    child = [sys.executable, os.path.abspath(__file__), "--full", "--no-cpu-baseline", "--no-mapping-build",
             "--no-secondary", "--no-pmc", "--steps", "1", "--warmup", "1",
             "--detail-file", os.path.join(work, "child_detail.json")]
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            out = os.path.join(work, f"pmc_{counter}")
            r = subprocess.run([exe, "--pmc", counter, "--kernel-trace", "-d", out, "-o", "pmc", "--output-format", "csv",
                                "--"] + child, cwd="/tmp", env=env, capture_output=True, text=True, timeout=timeout_s)
            hits = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not hits:
                _LIVE_PMC["why"] = f"rocprofv3 --pmc {counter} pass failed (rc {r.returncode}): {r.stderr[-200:]}"
                return
            want = os.path.join(out, "pmc_counter_collection.csv")
            if os.path.abspath(hits[0]) != want:
                shutil.copy(hits[0], want)
        sys.path.insert(0, os.path.join(ROOT, "profiles"))
        import summarize_pmc
        import contextlib
        import io
        dst = os.path.join(work, "pmc_traffic.json")
        with contextlib.redirect_stdout(io.StringIO()):
            summarize_pmc.main(work, dst)
        _LIVE_PMC["table"] = json.load(open(dst))
        _LIVE_PMC["why"] = None
        gout = os.path.join(ROOT, "gpurun_out")
        if os.path.isdir(gout):
            shutil.copy(dst, os.path.join(gout, "pmc_traffic_live.json"))
    except (subprocess.TimeoutExpired, OSError, KeyError, ValueError) as e:
        _LIVE_PMC["why"] = f"live PMC passes failed: {type(e).__name__}: {str(e)[:160]}"
    finally:
        shutil.rmtree(work, ignore_errors=True)


def _pmc_lookup(table, timer_name):
    sym = KERNEL_SYMBOL[timer_name]
    entry = table.get(sym)
    if entry is None:            # template arguments appended since the table of symbols was written: prefix match
        hits = [v for k, v in table.items() if k.startswith(sym.rstrip(">")) and isinstance(v, dict) and "hbm_bytes" in v]
        entry = max(hits, key=lambda v: v["hbm_bytes"]) if hits else None
    return entry


def pmc_traffic(timer_name, default_workload):
    """(HBM bytes per launch, reason) of the kernel from the committed rocprofv3 PMC passes of this same command
    (separate --pmc FETCH_SIZE / WRITE_SIZE runs, FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes;
    tools/gpu_evidence.sh + profiles/summarize_pmc.py).  Counters cannot be read from inside the process, so the
    value is only reported for the default workload the passes were taken on AND only when the file's stamp (sha256 of
    the kernel sources at the time of the passes) equals the hash of the sources this run is built from; otherwise
    (None, why)."""
    from deepviewagg_amd import _lib
    if not default_workload:
        return None, "not the workload the PMC passes were taken on"
    if timer_name in KERNEL_SYMBOL and _LIVE_PMC["table"] is not None:
        entry = _pmc_lookup(_LIVE_PMC["table"], timer_name)
        if entry is not None:
            return entry["hbm_bytes"], "live"
    if timer_name not in KERNEL_SYMBOL or not os.path.exists(PMC_TRAFFIC_FILE):
        return None, "no PMC pass for this kernel"
    table = json.load(open(PMC_TRAFFIC_FILE))
    stamp = (table.get("_stamp") or {}).get("csrc_sha256")
    if stamp != _lib.source_sha256():
        return None, (f"live passes: {_LIVE_PMC['why']}; profiles/pmc_traffic_latest.json is of other kernel sources "
                      f"(stamp {str(stamp)[:12]} != {_lib.source_sha256()[:12]})")
    entry = _pmc_lookup(table, timer_name)
    if entry is None:
        return None, f"kernel {KERNEL_SYMBOL[timer_name]} not in the PMC passes"
    return entry["hbm_bytes"], None


def step(scene, packed, mods, dtype, lazy=True, before_backward=None, interpolate=False):
    """One fused forward + backward of the hot path (metric M1 of SURVEY.md 8(d): gather -> atomic pool -> view
    attention pool -> fusion-concat).  The backward is seeded with a fixed upstream gradient [N, 4 + C] resident in
    HBM -- what the 3D backbone hands back -- so that no loss kernels sit inside the timed region.  Returns the
    fused features (detached)."""
    from deepviewagg_amd import ops
    atomic_pool, view_pool, fusion = mods
    x = scene["x"].requires_grad_(True)
    x.grad = None
    for p in view_pool.parameters():
        p.grad = None
    # mapping -> gather index (image.py:1871-1885 + downscale), rebuilt every step like the reference's
    # feature_map_indexing: the lazy path flattens (image, pixel) straight to map rows + the row plan (both are
    # functions of the mapping only); the materialised path goes through the packed 8-byte index
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=(dtype == torch.bfloat16)):
        # nearest gather, lazy: E_mod then runs on the map rows and the gather is fused into the attention kernel
        # (DESIGN.md "E_mod hoisting")
        exact = scene["pixels"].shape[0] == scene["x_map"].shape[0]
        if interpolate:
            # bilinear gather (image.py:1278-1283): coords = pixels / (mapping_size - 1) in (row, col) order
            packed = ops.pack_gather_index(scene["images"], scene["atom_ptr"], scene["pixels"], ratio=1.0)
            res = torch.tensor([scene["mapping_size"]], dtype=torch.float32, device=x.device)
            coords = (scene["pixels"] / (res - 1))[:, [1, 0]]
            x_mod = ops.lazy_gather_bilinear(x, packed, coords, exact) if lazy else ops.gather_bilinear(x, packed, coords)
        elif lazy:
            x_mod = ops.lazy_gather_nearest_mapping(x, scene["images"], scene["atom_ptr"], scene["pixels"], 1.0,
                                                    exact=exact)
        else:
            packed = ops.pack_gather_index(scene["images"], scene["atom_ptr"], scene["pixels"], ratio=1.0)
            x_mod = ops.gather_nearest(x, packed)
        x_mod = atomic_pool(None, x_mod, None, scene["atom_ptr"])             # identity for exact mappings
        x_pool = view_pool(scene["x_3d"], x_mod, scene["x_map"], scene["csr"])  # [N, C]
        out = fusion(scene["x_3d"], x_pool)                                   # [N, 4 + C] fp32 (cat promotes)
    if scene.get("grad_out") is None or scene["grad_out"].shape != out.shape:
        scene["grad_out"] = torch.randn(out.shape, device=out.device, dtype=out.dtype,
                                        generator=torch.Generator(device=out.device).manual_seed(99)) / out.shape[0]
    if before_backward is not None:
        before_backward()        # N > 1: the stand-in bucket's all-reduce starts on its side stream here
    out.backward(scene["grad_out"])
    return out.detach()


def cpu_baseline(log2_points, views, C, threads):
    """The oracle (plain PyTorch on the host cores) on a bounded sample of the same workload."""
    from oracle import pooling_oracle as O
    torch.set_num_threads(threads)
    n = 1 << log2_points
    g = torch.Generator().manual_seed(0)
    V = n * views
    csr = torch.arange(0, V + 1, views, dtype=torch.int64)
    images = torch.arange(views).repeat(n)
    H, W = 64, 128
    pixels = torch.stack([torch.randint(0, W, (V,), generator=g), torch.randint(0, H, (V,), generator=g)], 1)
    x = torch.randn(views, C, H, W, generator=g, requires_grad=True)
    x_map = torch.rand(V, 8, generator=g)
    x_3d = torch.randn(n, 4, generator=g)
    pool = O.GroupBimodalCSRPool(in_map=8, in_mod=C, num_groups=4, use_mod=False, map_encoder='DeepSetFeat',
                                 use_num=True).train()
    atom_ptr = torch.arange(V + 1)

    def one():
        xm = O.gather_nearest(x, images, pixels)
        xm = O.segment_csr(xm, atom_ptr, 'max')
        out = O.bimodal_fusion(x_3d, pool(None, xm, x_map, csr), 'concatenation')
        out.square().mean().backward()
    one()  # warm-up
    t0 = time.perf_counter()
    reps = 1
    for _ in range(reps):
        one()
    dt = (time.perf_counter() - t0) / reps
    return dict(value=n / dt, unit="points/s", cores=torch.get_num_threads(), cores_effective=1, kind="port",
                note="PyTorch-CPU restatement: bound by per-op dispatch and single-threaded index / segment ops (the "
                     "same rate on 8 and on 64 host threads), NOT a tuned multi-core implementation",
                sample=f"oracle/pooling_oracle.py (PyTorch CPU fp32), N=2^{log2_points} points x {views} views, "
                       f"C={C}, {reps} fwd+bwd steps, {dt:.2f} s/step")


def cpu_gather_attention_twin(log2_points, views, C, G=4):
    """The C + OpenMP twin of the view gather + attention tail (oracle/attention_oracle.c: softmax over the views of a
    point, gathered value rows, weighted group sum, gate; forward + backward incl. the rows scatter-add) on ALL host
    cores: the part of the path that is a CPU kernel rather than a PyTorch op sequence.  Bounded sample of S1."""
    import numpy as np
    from oracle import attention_oracle as A
    n = 1 << log2_points
    rng = np.random.default_rng(0)
    V, R = n * views, 32 * 64 * 128
    csr = np.arange(0, V + 1, views, dtype=np.int64)
    row_idx = rng.integers(0, R, V, dtype=np.int32)
    rows = rng.standard_normal((R, C), dtype=np.float32)
    compat = rng.standard_normal((V, G), dtype=np.float32)
    gw, gb = np.ones(G, np.float32), np.zeros(G, np.float32)
    gout = rng.standard_normal((n, C), dtype=np.float32)

    def one():
        out, att, gate, amax = A.forward(rows, row_idx, compat, csr, gw, gb, True)
        A.backward(gout, rows, row_idx, compat, csr, att, gate, amax, gw, gb, True)
    one()
    reps, t0 = 3, time.perf_counter()
    for _ in range(reps):
        one()
    dt = (time.perf_counter() - t0) / reps
    return dict(value=n / dt, unit="points/s", cores=A.num_threads(), kind="port",
                sample=f"oracle/attention_oracle.c (C + OpenMP, fp32), view gather + attention forward + backward only "
                       f"(no mapping-feature encoder, no E_mod), N=2^{log2_points} points x {views} views, C={C}, "
                       f"G={G}, {reps} steps, {dt:.3f} s/step",
                gpu_same_scope_note="on the GPU this scope is chain_attn_fwd + chain_attn_bwd + "
                                    "view_gather_rows_grad + row_plan (kernels table) minus the encoder recompute")


def _host_mem_available_gb():
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) / (1 << 20)
    except OSError:
        pass
    return 0.0


def cpu_full_path_twin(log2_points, views, C, G=4):
    """C + OpenMP twin of the WHOLE pooling step on all host cores (the build's own CPU restatement):
    E_mod on the map rows (count-weighted train-mode BatchNorm: oracle/deepset_oracle.c `oracle_wblock_*`), the
    mapping-feature encoder (DeepSetFeat + E_score, train-mode BatchNorm) feeding the view gather + attention tail
    (oracle/attention_oracle.c), the fusion concat; forward + backward incl. the rows scatter-add, E_mod's backward on the
    map rows and every parameter gradient.  Bounded sample of S1 (same shapes; N as large as the host memory allows)."""
    import numpy as np
    from oracle import attention_oracle as A
    from oracle import deepset_oracle as DS
    from oracle import pooling_oracle as O
    n = 1 << log2_points
    rng = np.random.default_rng(0)
    V, R = n * views, 32 * 64 * 128
    csr = np.arange(0, V + 1, views, dtype=np.int64)
    row_idx = rng.integers(0, R, V, dtype=np.int32)
    counts = np.bincount(row_idx, minlength=R).astype(np.float32)
    x_rows = rng.standard_normal((R, C), dtype=np.float32)
    x_map = rng.random((V, 8), dtype=np.float32)
    x_3d = rng.standard_normal((n, 4), dtype=np.float32)
    gw, gb = np.ones(G, np.float32), np.zeros(G, np.float32)
    gfused = rng.standard_normal((n, 4 + C), dtype=np.float32)
    torch.manual_seed(0)
    e_map, lin, e_mod = O.DeepSetFeat(8, 32, use_num=True), torch.nn.Linear(32, G), O.MLP([C, C, C], bias=False)
    P = DS.params_from_state_dict({k: v.detach().numpy() for k, v in e_map.state_dict().items()},
                                  lin.weight.detach().numpy(), lin.bias.detach().numpy())
    P_mod = DS.emod_params_from_state_dict({k: v.detach().numpy() for k, v in e_mod.state_dict().items()})

    def one():
        rows, mod_cache = DS.emod_forward(P_mod, x_rows, counts)
        scores, cache = DS.forward(P, x_map, csr, True)
        out, att, gate, amax = A.forward(rows, row_idx, scores, csr, gw, gb, True)
        fused = DS.fusion_concat_forward(x_3d, out)
        _, gout = DS.fusion_concat_backward(gfused, 4)
        g_rows, g_compat, _, _ = A.backward(gout, rows, row_idx, scores, csr, att, gate, amax, gw, gb, True)
        DS.backward(P, cache, g_compat)
        DS.emod_backward(P_mod, mod_cache, g_rows)
        return fused
    one()
    reps, t0 = 1 if log2_points >= 19 else 2, time.perf_counter()
    for _ in range(reps):
        one()
    dt = (time.perf_counter() - t0) / reps
    return dict(value=n / dt, unit="points/s", cores=DS.num_threads(), kind="port",
                sample=f"whole step fwd+bwd, C+OpenMP fp32 twin (oracle/deepset_oracle.c + attention_oracle.c), S1 shapes "
                       f"N=2^{log2_points} x {views} views, C={C}, {reps} step(s) after 1 warm-up, {dt:.2f} s/step",
                sample_long=f"oracle/deepset_oracle.c + oracle/attention_oracle.c (C + OpenMP, fp32, {DS.num_threads()} threads): "
                       f"E_mod on the {R} map rows -> DeepSetFeat + E_score (train-mode BatchNorm) -> view gather + attention "
                       f"-> fusion concat, forward + backward with every parameter gradient, S1 shapes at N=2^{log2_points} "
                       f"points x {views} views (V={V}), C={C}, G={G}, {reps} timed step(s) after one warm-up, "
                       f"{dt:.3f} s/step; the work is linear in V at fixed views per point, so points/s carries over to "
                       f"N=2^20 (N chosen by the host memory: ~2.3 KB of fp32 activations per view)")


def mapping_build_bench(device, n_images=32, n_points=200_000):
    """Secondary measurement: mapping build at the S3DIS settings (2048x1024 projection map,
    voxel 2 cm, r_max 8 m, exact=True), B = 32 cameras of one setting against a 200 k-point room: images/s of the
    BATCHED build (VisibilityModel.batch -> dva_visibility_batch: one set of launches, one host synchronisation) and
    of the image-by-image build, next to the C oracle on one host core, with a bit-exactness check of the indices."""
    import numpy as np
    from deepviewagg_amd.core.multimodal.visibility import SplattingVisibility
    from oracle import mapping_oracle as M
    rng = np.random.default_rng(0)
    face = rng.integers(0, 6, n_points)
    uvw = rng.random((n_points, 3))
    uvw[np.arange(n_points), face // 2] = face % 2
    xyz = (uvw * np.array([8.0, 6.0, 3.0])).astype(np.float32)
    cams = np.array([[3.1, 2.2, 1.4], [5.0, 3.0, 1.2], [2.0, 4.5, 1.6], [6.5, 1.5, 1.5]], dtype=np.float32)
    extra = (rng.random((max(n_images - 4, 0), 3)) * np.array([6.0, 4.0, 1.0]) + np.array([1.0, 1.0, 1.0])).astype(np.float32)
    cams = np.concatenate([cams, extra])[:n_images]
    W, H = 2048, 1024
    kw = dict(img_size=(W, H), r_max=8.0, r_min=0.05, voxel=0.02, k_swell=1.0, d_swell=1000, exact=True)
    model = SplattingVisibility(camera="s3dis_equirectangular", **kw)
    xyz_d = torch.from_numpy(xyz).to(device)
    cams_d = torch.from_numpy(cams).to(device)
    opk = torch.zeros(3, device=device)
    opk_b = torch.zeros((n_images, 3), device=device)
    # ---- batched
    out = model.batch(xyz_d, cams_d, img_opk=opk_b)          # warm-up
    torch.cuda.synchronize()
    reps = 5
    t0 = time.perf_counter()
    for _ in range(reps):
        out = model.batch(xyz_d, cams_d, img_opk=opk_b)
    torch.cuda.synchronize()
    batch_s = (time.perf_counter() - t0) / (reps * n_images)
    # ---- image by image (4 images)
    single = [model(xyz_d, cams_d[i], img_opk=opk) for i in range(4)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        single = [model(xyz_d, cams_d[i], img_opk=opk) for i in range(4)]
    torch.cuda.synchronize()
    gpu_s = (time.perf_counter() - t0) / (reps * 4)
    cam0 = M.make_camera("s3dis_equirectangular", kw["img_size"], cams[0], r_min=kw["r_min"], r_max=kw["r_max"],
                         voxel=kw["voxel"], k_swell=1.0, d_swell=1000, exact=True, img_opk=np.zeros(3))
    t0 = time.perf_counter()
    ref = M.visibility(xyz, cam0)
    cpu_s = time.perf_counter() - t0
    rp = out["row_ptr"].cpu().numpy()
    exact = all(bool(np.array_equal(out[k][rp[0]:rp[1]].cpu().numpy(), ref[k])) for k in ("idx", "x", "y")) and \
        all(bool(torch.equal(out[k][rp[i]:rp[i + 1]], single[i][k])) for i in range(4) for k in ("idx", "x", "y"))
    # SURVEY.md 8(d) bytes per image: n 12 B of xyz read + W_p H_p 12 B of z-buffer / pixel map cleared and scanned
    # + 8 B per pixel of every splat box (the z-buffer atomics); the box areas from the splat formula (visibility.py:651-704)
    area = 0
    for c in cams:
        v = xyz - c
        d = np.sqrt((v * v).sum(1))
        ok = (d > kw["r_min"]) & (d < kw["r_max"])
        v, d = v[ok].astype(np.float64), d[ok].astype(np.float64)
        y = (H - 1) * np.arccos(np.clip(v[:, 2] / d, -1, 1)) / np.pi
        a = (1.0 + np.exp(-d / np.log(1000.0))) * kw["voxel"] / d
        wy = a * H / np.pi
        wx = (a * W / (2 * np.pi)) / (np.sin(np.pi * y / H) + 0.001)
        area += float((np.minimum(np.rint(wx + 1), W) * np.minimum(np.rint(wy + 1), H)).sum())
    per_image = n_points * 12 + W * H * 12 + area / len(cams) * 8
    return {"roofline": {"bound": "hbm", "algorithmic_bytes_per_image": per_image,
                         "splat_box_pixels_per_image": area / len(cams), "achieved": per_image / batch_s / 1e9,
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": per_image / batch_s / 1e9 / HBM_PEAK_GBS,
                         "note": "tiled z-buffer (survivors binned into 32 x 32 screen tiles, one workgroup per tile, "
                                 "z-buffer in LDS), exact re-splat, block-count emit: bound by the scattered atomics of "
                                 "binning / re-splat and the fixed map-sized passes, not by HBM bandwidth"},
            "images_per_s": 1.0 / batch_s, "ms_per_image": batch_s * 1e3, "batch": n_images,
            "single_image_calls": {"images_per_s": 1.0 / gpu_s, "ms_per_image": gpu_s * 1e3},
            "candidates_per_image": n_points, "proj_map": [W, H], "mapped_points_image0": int(ref["idx"].shape[0]),
            "cpu_oracle_ms_per_image_1core": cpu_s * 1e3, "indices_bit_exact_vs_oracle": exact}


def copy_ceiling(device, nbytes=1 << 32, reps=5):
    """Practical HBM ceiling: read + write rate of the library's device copy (dva_copy_ceiling: a chunk per
    block, non-temporal 16-byte loads / stores) over `nbytes`; MI355X_MICROARCH.md measures 6.29 TB/s for this pattern."""
    from deepviewagg_amd import _lib
    lib = _lib.load()
    src = torch.empty(nbytes, dtype=torch.uint8, device=device)
    dst = torch.empty_like(src)
    st = _lib.stream_of(src)
    _lib.check(lib.dva_copy_ceiling(_lib.ptr(src), _lib.ptr(dst), nbytes, st), "dva_copy_ceiling")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        _lib.check(lib.dva_copy_ceiling(_lib.ptr(src), _lib.ptr(dst), nbytes, st), "dva_copy_ceiling")
    e1.record()
    torch.cuda.synchronize()
    return 2.0 * nbytes * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9


def gather_bench(scene, reps=5):
    """Metric M2 of SURVEY.md 8(d): the materialised nearest view gather (image.py:1285) at the scene's V --
    GB/s on the algorithmic bytes  P (C s + idx) read + P C s written  (the fused path never runs this kernel)."""
    from deepviewagg_amd import ops
    x = scene["x"].detach()
    packed = ops.pack_gather_index(scene["images"], scene["atom_ptr"], scene["pixels"], ratio=1.0)
    out = ops.gather_nearest(x, packed)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = ops.gather_nearest(x, packed)
    e1.record()
    torch.cuda.synchronize()
    P, C = out.shape
    nbytes = P * (2 * C * out.element_size() + 8)
    ms = e0.elapsed_time(e1) / reps
    del out
    return {"GBps": nbytes / (ms * 1e-3) / 1e9, "ms": ms, "atoms": P, "bytes": nbytes}


PROFILE_STEPS = 2     # untimed steps with HIP events around EVERY launch: the per-kernel tables


def timed_steps(scene, mods, dtype, steps, warmup, lazy=True, interpolate=False):
    """`steps` timed steps of one workload on the current device (secondary workloads; no collectives): wall time of the
    steps WITHOUT per-launch events (an event pair costs ~6 us of stream bubble: 8 % of a 3.5 ms step), then
    PROFILE_STEPS more steps with events around every launch for the per-kernel table."""
    from deepviewagg_amd import ops
    for _ in range(warmup):
        step(scene, None, mods, dtype, lazy=lazy, interpolate=interpolate)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step(scene, None, mods, dtype, lazy=lazy, interpolate=interpolate)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    sanity = sanity_values(out, scene["x"].grad)
    ops.TIMER = ops.KernelTimer()
    for _ in range(PROFILE_STEPS):
        step(scene, None, mods, dtype, lazy=lazy, interpolate=interpolate)
    timer, ops.TIMER = ops.TIMER, None
    kern = timer.summary()
    kern["__sanity__"] = sanity
    return ms, kern


def timed_steps_guarded(scene, mods, dtype, steps, warmup, interpolate=False):
    """timed_steps, timed once more when the wall time is far above the sum of the timed kernels: a warm-up artefact
    (allocator growth after the previous workload's buffers were released was seen to double a C = 512 step once; a 3 s
    host stall inside one 5-step region was seen once in round 6: kitti 128 -> 64 at 636 ms/step instead of 22)."""
    ms, kern = timed_steps(scene, mods, dtype, steps, warmup, interpolate=interpolate)
    sanity = kern.pop("__sanity__")
    retimed = False
    if ms > 1.25 * sum(v["ms"] for v in kern.values()) / PROFILE_STEPS + 3.0:
        ms2, kern2 = timed_steps(scene, mods, dtype, steps, 0, interpolate=interpolate)
        kern2.pop("__sanity__")
        if ms2 < ms:
            ms, kern, retimed = ms2, kern2, True
    return ms, kern, sanity, retimed


def sanity_values(out, x_grad):
    """What the last timed step computed (a timing of an unverified computation is not a measurement):
    mean |.| and finiteness of the fused features and of the feature-map gradient, outside the timed region."""
    o, g = out.float(), x_grad.float()
    return {"out_abs_mean": float(o.abs().mean()), "out_finite": bool(torch.isfinite(o).all()),
            "grad_x_abs_mean": float(g.abs().mean()), "grad_x_finite": bool(torch.isfinite(g).all()),
            "grad_x_rows_nonzero_frac": float((g.abs().sum(1) > 0).float().mean()) if g.dim() == 4 else None}


def fused_fwd_bytes(V, N, C, es):
    """SURVEY.md 8(d) 'fused view-gather + attention' forward minimum: V (g C s + F_map 4 + idx) + N (C s + ptr),
    g = 1 (nearest), idx = 8 bytes / view (here: view -> point index + row index), ptr = 8 bytes / point."""
    return V * (C * es + 32 + 8) + N * (C * es + 8)


def fused_bwd_bytes(V, N, C, es, G=4):
    """Attention backward on the same accounting: per view the gathered row, the stored scores (16), the indices (8), the
    score gradients written (16) and the 16-byte record of the rows-gradient pass; per point the grad_out row."""
    return V * (C * es + 16 + 8 + 16 + 16) + N * (C * es + 8)


def secondary_workload(name, device, dtype, log2_points, views, C, steps=10, warmup=2, interpolate=False, C_out=None):
    """One secondary workload of SURVEY.md 8(d) (S2: ragged view counts; F-L: C = 512, value map > MALL; bilinear:
    interpolate=True with the mapping at 8 x the map resolution): ms/step and the roofline fractions of the fused view
    kernel (forward) and of the attention backward kernel."""
    wl = name if name in ("S2", "S1c") else "S1"
    N = 1 << log2_points
    scene = make_scene(N, views, 32, C, 64, 128, dtype, device, seed=4321, workload=wl, upscale=8 if interpolate else 1)
    mods = build_modules(C, device, C_out, pool="qkv" if name == "qkv" else "group")
    ms, kern, sanity, retimed = timed_steps_guarded(scene, mods, dtype, steps, warmup, interpolate=interpolate)
    if interpolate:
        # the fused bilinear path against the reference's materialised [V, C] dataflow on the same scene (same
        # parameters: its sanity values are the yardstick of the fused path's)
        ms_mat, kern_mat = timed_steps(scene, mods, dtype, 3, 1, lazy=False, interpolate=True)
        sanity_mat = kern_mat.pop("__sanity__")
        top = sorted(kern.items(), key=lambda kv: -kv[1]["ms"])[:6]
        out = {"points": N, "views": int(scene["x_map"].shape[0]), "channels": C, "out_channels": C_out or C,
               "ms_per_step": ms, "points_per_s": N / (ms * 1e-3), "fused_path": "emod_attn_fwd" in kern,
               "materialised_ms_per_step": ms_mat, "speedup_vs_materialised": ms_mat / ms,
               "steps": steps, "sanity": sanity, "sanity_materialised": sanity_mat,
               "top_kernels_ms": {n: v["ms"] / v["launches"] for n, v in top}}
        del scene, mods
        torch.cuda.empty_cache()
        return out
    V = int(scene["x_map"].shape[0])
    es = 2 if dtype == torch.bfloat16 else 4
    out = {"points": N, "views": V, "channels": C, "ms_per_step": ms, "points_per_s": N / (ms * 1e-3), "steps": steps,
           "sanity": sanity, "retimed": retimed}
    for key, nbytes in (("chain_attn_fwd", fused_fwd_bytes(V, N, C, es)), ("chain_attn_bwd", fused_bwd_bytes(V, N, C, es))):
        k = kern.get(key)
        if k is not None:
            t = k["ms"] / k["launches"]
            out[key] = {"avg_launch_ms": t, "algorithmic_bytes": nbytes, "GBps": nbytes / (t * 1e-3) / 1e9,
                        "frac_of_hbm_peak": nbytes / (t * 1e-3) / 1e9 / HBM_PEAK_GBS}
    top = sorted(kern.items(), key=lambda kv: -kv[1]["ms"])[:4 if name not in ("f32", "qkv") else 12]
    out["top_kernels_ms"] = {n: v["ms"] / v["launches"] for n, v in top}
    if name == "S1c":
        k = kern.get("view_gather_rows_grad")
        out["view_gather_rows_grad_ms"] = k["ms"] / k["launches"] if k else None
        out["note"] = ("locality probe, not a SURVEY workload: S1 with projection-like pixels (neighbouring points hit "
                       "neighbouring pixels, as in a real scan) -- what the random-pixel S1 costs the rows gradient")
    if name == "f32":
        out["dtype"] = "f32"
        out["scores_path"] = "chain3" if any(k.startswith("chain3_") for k in kern) else "stored activations"
    del scene, mods
    torch.cuda.empty_cache()
    return out


def two_setting_bilinear_workload(device, log2_points=20, views=32, C=64, steps=5, warmup=2):
    """A multi-setting batch on the bilinear path: ImageData = two settings with different map sizes
    (16 maps [C, 64, 128] and 16 maps [C, 32, 64]); every point is seen by views / 2 images of each, the views of the two
    settings are concatenated and brought into point order (the reference's view_cat_sorting, core/multimodal/image.py:
    1549-1588).  Lazy: ONE concatenated tap gather through fused_bilinear (ops.InterpolatedFeatures.cat); materialised:
    the reference's dataflow (two [V_s, C] gathers, cat, index)."""
    from deepviewagg_amd import ops
    N, k = 1 << log2_points, views // 2
    g = torch.Generator(device=device).manual_seed(2468)
    geo = [(16, 64, 128), (16, 32, 64)]
    up = 8
    xs, packs, coords = [], [], []
    for B, H, W in geo:
        Vs = N * k
        images = torch.arange(B, device=device)[:k].repeat(N) if k <= B else None
        pixels = torch.stack([torch.randint(0, W * up, (Vs,), generator=g, device=device),
                              torch.randint(0, H * up, (Vs,), generator=g, device=device)], 1).to(torch.int16)
        xs.append(torch.randn(B, C, H, W, generator=g, device=device).bfloat16().contiguous(memory_format=torch.channels_last))
        packs.append(ops.pack_gather_index(images.long(), torch.arange(Vs + 1, device=device), pixels, ratio=1.0))
        res = torch.tensor([[W * up, H * up]], dtype=torch.float32, device=device)
        coords.append((pixels / (res - 1))[:, [1, 0]].contiguous())
    V = 2 * N * k
    pt = torch.arange(N, device=device).view(-1, 1)
    j = torch.arange(k, device=device).view(1, -1)
    order = torch.cat([pt * k + j, N * k + pt * k + j], dim=1).reshape(-1)        # point order: setting A's views, then B's
    csr = torch.arange(0, V + 1, 2 * k, dtype=torch.int64, device=device)
    x_map = torch.rand(V, 8, generator=g, device=device)
    x_3d = torch.randn(N, 4, generator=g, device=device)
    atomic_pool, view_pool, fusion = build_modules(C, device)
    grad_out = None

    def one(lazy):
        nonlocal grad_out
        for x in xs:
            x.requires_grad_(True)
            x.grad = None
        for p_ in view_pool.parameters():
            p_.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            parts = [ops.lazy_gather_bilinear(x, pk, co, True) for x, pk, co in zip(xs, packs, coords)]
            if lazy:
                x_mod = ops.InterpolatedFeatures.cat(parts, order=order)
            else:
                x_mod = torch.cat([p_.materialize() for p_ in parts], dim=0)[order]
            out = fusion(x_3d, view_pool(x_3d, x_mod, x_map, csr))
        if grad_out is None:
            grad_out = torch.randn(out.shape, device=device, dtype=out.dtype,
                                   generator=torch.Generator(device=device).manual_seed(99)) / out.shape[0]
        out.backward(grad_out)
        return out.detach()

    def timed(lazy, n, w):
        for _ in range(w):
            one(lazy)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            out = one(lazy)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, sanity_values(out, xs[0].grad)
    ms, sanity = timed(True, steps, warmup)
    ops.TIMER = ops.KernelTimer()
    one(True)
    timer, ops.TIMER = ops.TIMER, None
    kern = timer.summary()
    ms_mat, sanity_mat = timed(False, 2, 1)
    top = sorted(kern.items(), key=lambda kv: -kv[1]["ms"])[:6]
    out = {"points": N, "views": V, "settings": [list(g_) for g_ in geo], "channels": C, "ms_per_step": ms,
           "points_per_s": N / (ms * 1e-3), "fused_path": "emod_attn_fwd" in kern, "materialised_ms_per_step": ms_mat,
           "speedup_vs_materialised": ms_mat / ms, "steps": steps, "sanity": sanity, "sanity_materialised": sanity_mat,
           "top_kernels_ms": {n: v["ms"] / v["launches"] for n, v in top}}
    del xs, packs, coords, x_map
    torch.cuda.empty_cache()
    return out


def make_s3dis_batch_scene(device, dtype=torch.bfloat16, samples=4, points_per_sample=75_000, images_per_sample=4,
                           C=512, H=64, W=128, seed=77):
    """A batch the size the reference actually trains S3DIS on (BASELINE config 1): `batch_size: 4` spheres
    (conf/data/segmentation/multimodal/s3disfused-sparse.yaml:108-109 sample_per_epoch / scripts/train_s3dis.sh:23-24),
    pixel credit of 4 images per sample (:153-156), ADE20K ResNet18 layer-4 feature maps [512, 64, 128] -- so a point is seen
    by at most the 4 images of its own sphere: k_i = 0 (10 % unseen) or 1 + Binomial(3, 3/4), V ~ 8.8e5 views over
    3e5 points, 16 feature maps.  Exact mapping (one pixel per view), pixels uniform."""
    g = torch.Generator(device=device).manual_seed(seed)
    n = samples * points_per_sample
    k = 1 + (torch.rand(n, 3, generator=g, device=device) < 0.75).sum(1)
    k[torch.rand(n, generator=g, device=device) < 0.1] = 0
    csr = torch.cat([torch.zeros(1, dtype=torch.int64, device=device), k.cumsum(0)])
    V = int(csr[-1])
    pt = torch.arange(n, device=device).repeat_interleave(k)
    rank = torch.arange(V, device=device) - csr[:-1].repeat_interleave(k)
    # the k_i images of a point: a random cyclic run of its sphere's images, sorted inside the point (from_dense order)
    start = torch.randint(0, images_per_sample, (n,), generator=g, device=device)[pt]
    img_local = (start + rank) % images_per_sample
    images = (pt // points_per_sample) * images_per_sample + img_local
    images = images[torch.argsort(pt * (samples * images_per_sample) + images)]
    pixels = torch.stack([torch.randint(0, W, (V,), generator=g, device=device),
                          torch.randint(0, H, (V,), generator=g, device=device)], 1).to(torch.int16)
    x = torch.randn(samples * images_per_sample, C, H, W, generator=g, device=device).to(dtype)
    x = x.contiguous(memory_format=torch.channels_last)
    return dict(csr=csr, images=images.long(), pixels=pixels, atom_ptr=torch.arange(V + 1, dtype=torch.int64, device=device),
                x=x, x_map=torch.rand(V, 8, generator=g, device=device), x_3d=torch.randn(n, 4, generator=g, device=device),
                mapping_size=(W, H))


def nonexact_workload(device, log2_points=18, views=32, pixels_per_view=4, C=64, steps=5, warmup=2):
    """VERDICT r3 missing 3: a NON-exact mapping (exact_splatting_2d off: several pixels per view, reference
    core/multimodal/visibility.py:1168-1187 -> modules/multimodal/modules.py:400-407 atomic max pool): 2^18 points x 32
    views x 4 pixels (P = 33.5 M atoms), C = 64, train mode fwd + bwd.  Lazy route (round 4): gather + atomic max pool in
    one kernel, no [P, C] tensor, pooled [V, C] rows handed to the recompute chain; materialised route: the reference's
    dataflow ([P, C] gather, segment max, view pooling on the [V, C] tensor)."""
    from deepviewagg_amd import ops
    dtype = torch.bfloat16
    N = 1 << log2_points
    scene = make_scene(N, views, 32, C, 64, 128, dtype, device, seed=4321)
    V = scene["x_map"].shape[0]
    g = torch.Generator(device=device).manual_seed(17)
    P = V * pixels_per_view
    scene["pixels"] = torch.stack([torch.randint(0, 128, (P,), generator=g, device=device),
                                   torch.randint(0, 64, (P,), generator=g, device=device)], 1).to(torch.int16)
    scene["atom_ptr"] = torch.arange(0, P + 1, pixels_per_view, dtype=torch.int64, device=device)
    out = {"points": N, "views": V, "atoms": P, "channels": C}
    for name, lazy_route in (("lazy", True), ("materialised", False)):
        ops.LAZY_NONEXACT = lazy_route
        try:
            mods = build_modules(C, device)
            ms, kern = timed_steps(scene, mods, dtype, steps, warmup)
        finally:
            ops.LAZY_NONEXACT = True
        sanity = kern.pop("__sanity__")
        out[name] = {"ms_per_step": ms, "sanity": sanity,
                     "top_kernels_ms": {k: v["ms"] / v["launches"] for k, v in
                                        sorted(kern.items(), key=lambda kv: -kv[1]["ms"])[:6]}}
        del mods
        torch.cuda.empty_cache()
    out["ms_per_step"] = out["lazy"]["ms_per_step"]
    out["speedup_vs_materialised"] = out["materialised"]["ms_per_step"] / out["lazy"]["ms_per_step"]
    return out


def s3dis_batch_workload(device, steps=30, warmup=5, graph=True):
    """the hot path at the reference's own training-batch size, where the Python front end -- not the
    GPU -- could be the bottleneck: eager ms/step, the host's enqueue time per step, and the same step captured once in a
    torch.cuda.CUDAGraph (= hipGraph) and replayed (the GPU-bound time of the identical kernel sequence)."""
    dtype = torch.bfloat16
    scene = make_s3dis_batch_scene(device, dtype)
    mods = build_modules(512, device)
    N, V = scene["x_3d"].shape[0], scene["x_map"].shape[0]

    def one():
        return step(scene, None, mods, dtype, lazy=True)
    for _ in range(warmup):
        one()
    torch.cuda.synchronize()
    enq = 0.0
    t0 = time.perf_counter()
    for _ in range(steps):
        t1 = time.perf_counter()
        out = one()
        enq += time.perf_counter() - t1
    torch.cuda.synchronize()
    eager = (time.perf_counter() - t0) / steps * 1e3
    g_eager = scene["x"].grad.clone()
    res = {"points": N, "views": V, "feature_maps": list(scene["x"].shape), "ms_per_step_eager": eager,
           "host_enqueue_ms_per_step": enq / steps * 1e3, "points_per_s_eager": N / (eager * 1e-3), "steps": steps,
           "sanity": sanity_values(out, scene["x"].grad)}
    if not graph:
        return res
    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                one()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        scene["x"].grad = None
        with torch.cuda.graph(graph):
            one()
        torch.cuda.synchronize()
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            graph.replay()
        torch.cuda.synchronize()
        replay = (time.perf_counter() - t0) / steps * 1e3
        g_cap = scene["x"].grad
        res.update({"ms_per_step_graph_replay": replay, "points_per_s_graph_replay": N / (replay * 1e-3),
                    "graph_vs_eager_max_rel_grad_difference":
                        float((g_cap.float() - g_eager.float()).abs().max() / (g_eager.float().abs().max() + 1e-30)),
                    "host_bound_eager": eager > 1.15 * replay})
        del graph
    except Exception as e:                                  # capture is an optimisation: the eager number stands
        res["graph_error"] = f"{type(e).__name__}: {e}"[:300]
    del scene, mods
    torch.cuda.empty_cache()
    return res


def kitti360_pyramid_eval(device, log2_points, views, steps=10):
    """Inference (eval mode, no_grad) of the view pooling over the five pyramid levels of the reference's published
    KITTI-360 model (conf/models/segmentation/multimodal/sparseconv3d.yaml:7281-7290: in_mod -> out_mod = 128 -> 32,
    64 -> 32, 128 -> 64, 256 -> 128, 512 -> 256, interpolate=True, G = 4) at the S1 scene size: ms per forward and
    level, all five on the one fused kernel (bilinear taps of Linear_a(x) -> E_mod -> attention -> pooled features)."""
    from deepviewagg_amd import ops, fused_bilinear
    N = 1 << log2_points
    out = {"points": N, "views": N * views, "levels": {}}
    total = 0.0
    for C, Co in ((128, 32), (64, 32), (128, 64), (256, 128), (512, 256)):
        scene = make_scene(N, views, 32, C, 64, 128, torch.bfloat16, device, seed=4321, workload="S1", upscale=8)
        atomic_pool, view_pool, fusion = build_modules(C, device, Co)
        view_pool.eval()
        used = []
        orig = fused_bilinear.pool

        def spy(*a, **k):
            used.append(1)
            return orig(*a, **k)

        def forward():
            x = scene["x"]
            with torch.autocast("cuda", dtype=torch.bfloat16):
                packed = ops.pack_gather_index(scene["images"], scene["atom_ptr"], scene["pixels"], ratio=1.0)
                res = torch.tensor([scene["mapping_size"]], dtype=torch.float32, device=x.device)
                coords = (scene["pixels"] / (res - 1))[:, [1, 0]]
                x_mod = ops.lazy_gather_bilinear(x, packed, coords, True)
                x_mod = atomic_pool(None, x_mod, None, scene["atom_ptr"])
                return fusion(scene["x_3d"], view_pool(scene["x_3d"], x_mod, scene["x_map"], scene["csr"]))
        fused_bilinear.pool = spy
        try:
            with torch.no_grad():
                forward()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    o = forward()
                torch.cuda.synchronize()
        finally:
            fused_bilinear.pool = orig
        ms = (time.perf_counter() - t0) / steps * 1e3
        total += ms
        o = o.float()
        out["levels"][f"{C}_to_{Co}"] = {"ms": ms, "fused_kernel": len(used) == steps + 1, "steps": steps,
                                         "out_abs_mean": float(o.abs().mean()),
                                         "out_finite": bool(torch.isfinite(o).all())}
        del o
        del scene, atomic_pool, view_pool, fusion
        torch.cuda.empty_cache()
    out["ms_all_levels"] = total
    out["points_per_s"] = N / (total * 1e-3)
    return out


def kitti360_pyramid_train(device, log2_points, views, steps=5):
    """Training step (train mode, forward + backward) of the view pooling over the five pyramid levels of the reference's
    published KITTI-360 model (conf/models/segmentation/multimodal/sparseconv3d.yaml:7281-7290, interpolate=True, G = 4)
    at the S1 scene size: all five levels on the fused bilinear path (C_out = 128 / 256: the block-by-block kernels of round
    4).  Per level: ms/step, whether the fused path ran, sanity values; for the two wide levels also the reference's
    materialised dataflow ([V, C_in] gather + per-view E_mod) on the same scene and its sanity values as the yardstick."""
    N = 1 << log2_points
    out = {"points": N, "views": N * views, "levels": {}}
    total = 0.0
    for C, Co in ((128, 32), (64, 32), (128, 64), (256, 128), (512, 256)):
        scene = make_scene(N, views, 32, C, 64, 128, torch.bfloat16, device, seed=4321, workload="S1", upscale=8)
        mods = build_modules(C, device, Co)
        ms, kern, sanity, retimed = timed_steps_guarded(scene, mods, torch.bfloat16, steps, 2, interpolate=True)
        top = sorted(kern.items(), key=lambda kv: -kv[1]["ms"])[:8]
        lvl = {"ms_per_step": ms, "fused_path": "emod_attn_fwd" in kern, "steps": steps, "sanity": sanity, "retimed": retimed,
               "top_kernels_ms": {n: v["ms"] / v["launches"] for n, v in top}}
        if Co >= 128:
            ms_mat, kern_mat = timed_steps(scene, mods, torch.bfloat16, 2, 1, lazy=False, interpolate=True)
            lvl["materialised_ms_per_step"] = ms_mat
            lvl["speedup_vs_materialised"] = ms_mat / ms
            lvl["sanity_materialised"] = kern_mat.pop("__sanity__")
        out["levels"][f"{C}_to_{Co}"] = lvl
        total += ms
        del scene, mods
        torch.cuda.empty_cache()
    out["ms_all_levels"] = total
    out["points_per_s"] = N / (total * 1e-3)
    return out


def neighborhood_bench(device, n_points=1 << 20, k=50, n_images=32, views_per_point=8):
    """Secondary measurement: K-NN (k = 50, the S3DIS setting) over a 1M-point
    surface cloud + per-view occlusion, next to an exact KD-tree (scipy, 1 host core) on a 2^15-point sample
    of the same cloud."""
    import numpy as np
    from deepviewagg_amd import ops
    g = torch.Generator(device="cpu").manual_seed(0)
    face = torch.randint(0, 3, (n_points,), generator=g)
    xyz = torch.rand(n_points, 3, generator=g) * torch.tensor([8.0, 6.0, 3.0])
    lim = torch.tensor([8.0, 6.0, 3.0])[face]
    xyz[torch.arange(n_points), face] = torch.randint(0, 2, (n_points,), generator=g).float() * lim
    xyz = (xyz + torch.randn(n_points, 3, generator=g) * 1e-3).to(device)
    ops.knn(xyz[:4096], k)                                   # warm-up (rocPRIM kernels, allocator)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nbr, d2 = ops.knn(xyz, k)
    torch.cuda.synchronize()
    knn_s = time.perf_counter() - t0
    V = n_points * views_per_point
    csr = torch.arange(0, V + 1, views_per_point, device=device)
    images = torch.randint(0, n_images, (V,), generator=g).to(device)
    ops.view_occlusion(csr, images, nbr, [k], n_images)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.view_occlusion(csr, images, nbr, [k], n_images)
    torch.cuda.synchronize()
    occ_s = time.perf_counter() - t0
    from scipy.spatial import cKDTree
    sample = xyz[: 1 << 15].cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    dist, _ = cKDTree(sample).query(sample, k=k)
    cpu_s = time.perf_counter() - t0
    nb_s, d2_s = ops.knn(xyz[: 1 << 15], k)
    same = bool(np.allclose(np.sqrt(d2_s.cpu().numpy().astype(np.float64)), dist, rtol=1e-4, atol=1e-6))
    # roofline: algorithmic bytes = every point read once as a query and once as a candidate of its
    # cell (2 x 16 B) + k x (8 B index + 4 B distance) written; the search itself is bound by the distance evaluations
    # of the candidates in the 27+ cells around a query, not by HBM
    knn_bytes = n_points * (32 + k * 12)
    return {"points": n_points, "k": k, "knn_ms": knn_s * 1e3, "knn_points_per_s": n_points / knn_s,
            "roofline": {"bound": "hbm", "algorithmic_bytes": knn_bytes, "achieved": knn_bytes / knn_s / 1e9,
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": knn_bytes / knn_s / 1e9 / HBM_PEAK_GBS,
                         "note": "far below the HBM roofline by construction: an exact k = 50 search evaluates a few "
                                 "hundred candidate distances per query out of cell lists that sit in L2; the kernel "
                                 "is bound by those evaluations and the k-selection, its algorithmic bytes are 632 per "
                                 "point"},
            "occlusion_views": V, "occlusion_ms": occ_s * 1e3,
            "cpu_kdtree_points_per_s_1core": (1 << 15) / cpu_s, "cpu_sample": "scipy cKDTree, 2^15 points, k=50",
            "kth_distances_match_kdtree": same}


def tile_of_scene(scene, rank, world):
    """Strong scaling: the spatial tile `rank` of `world` of a scene (points by x-y slab of a synthetic raster,
    the views of a point travel with the point, the feature maps are replicated: SURVEY.md 8(e))."""
    from deepviewagg_amd.parallel import tile_partition, shard_mapping
    N = scene["csr"].shape[0] - 1
    side = int(round(N ** 0.5))
    pid = torch.arange(N, device=scene["csr"].device)
    xyz = torch.stack([(pid % side).float(), (pid // side).float(), torch.zeros_like(pid).float()], 1)
    pts = tile_partition(xyz, world)[rank]
    csr_t, views = shard_mapping(scene["csr"], pts)
    out = dict(scene)
    out.update(csr=csr_t, images=scene["images"][views], pixels=scene["pixels"][views].contiguous(),
               atom_ptr=torch.arange(views.shape[0] + 1, dtype=torch.int64, device=views.device),
               x_map=scene["x_map"][views].contiguous(), x_3d=scene["x_3d"][pts].contiguous())
    return out


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(args):
    """`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment: this process becomes the launcher.
    It re-executes this same command line under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N
    --master-addr 127.0.0.1` (one rank per GPU, LOCAL_RANK = device ordinal) and passes the ranks' output and exit
    code through; rank 0 prints the JSON line.  (The driver's own torchrun launch sets WORLD_SIZE and never gets here.)"""
    import subprocess
    port = os.environ.get("MASTER_PORT") or str(_free_port())
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")    # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 1) // args.gpus)))
    print(f"bench.py: launching {args.gpus} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    return subprocess.call(cmd, env=env)


def rank_census(world, rank, local_rank, device, backend):
    """All-gather of (rank, device ordinal) over the process group: the ranks really are `world` distinct processes and,
    under RCCL, sit on `world` distinct devices.  Returns the list of (rank, device) pairs."""
    assert dist.get_world_size() == world and dist.get_backend() == backend
    who = torch.tensor([rank, local_rank], device=device, dtype=torch.int64)
    gathered = [torch.empty_like(who) for _ in range(world)]
    dist.all_gather(gathered, who)
    ranks_devices = [tuple(int(v) for v in g.tolist()) for g in gathered]
    assert sorted(r for r, _ in ranks_devices) == list(range(world)), ranks_devices
    assert len({d for _, d in ranks_devices}) == world, f"ranks share a device: {ranks_devices}"
    return ranks_devices


DETAIL_FILE = "bench_detail.json"
LINE_HARD_CAP = 8192      # the driver keeps an 8 KB tail of stdout: a longer line cannot be parsed (BENCH_r05: parsed = null)
LINE_TARGET = 4096


def _sig(v, digits=5):
    """Floats at `digits` significant digits (a measurement record, not a dump of doubles)."""
    if isinstance(v, float):
        return float(f"{v:.{digits}g}")
    if isinstance(v, dict):
        return {k: _sig(x, digits) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_sig(x, digits) for x in v]
    return v


def _clip(s, n):
    return s if s is None or len(s) <= n else s[: n - 3] + "..."


def _roofline_compact(r):
    if not r:
        return None
    keys = ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "launches",
            "algorithmic_bytes_per_launch", "frac_of_copy_ceiling")
    out = {k: r[k] for k in keys if k in r}
    if "traffic_source" in r:
        out["traffic_source"] = _clip(r["traffic_source"], 120)
    return out


def _workload_ms(w):
    for k in ("ms_per_step", "ms_all_levels", "ms_per_step_eager"):
        if isinstance(w, dict) and k in w:
            v = w[k]
            return v.get("lazy") if isinstance(v, dict) else v
    return None


def compact_line(res, detail_file=DETAIL_FILE):
    """The ONE stdout line: the contract fields, the two roofline objects and, after --full, cpu_baseline and one number
    per secondary measurement.  Everything else (`workloads`, the full per-kernel table, per-step arrays, mapping build detail, prose
    notes) lives in `detail_file`.  tests/test_bench_line.py holds the size cap."""
    contract = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data")
    line = {k: res.get(k) for k in contract}
    cfg = dict(res.get("config") or {})
    cfg["workload"] = _clip(cfg.get("workload"), 420)
    ga = cfg.get("gradient_allreduce")
    if ga:
        cfg["gradient_allreduce"] = {k: v for k, v in ga.items() if k != "note"}
    line["config"] = cfg
    line["roofline"] = _roofline_compact(res.get("roofline"))
    line["roofline_view_gather_attention"] = _roofline_compact(res.get("roofline_view_gather_attention"))
    cb = res.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = ({"error": _clip(cb["error"], 200)} if "error" in cb else
                                {"value": cb.get("value"), "unit": cb.get("unit"), "cores": cb.get("cores"),
                                 "kind": cb.get("kind"), "sample": _clip(cb.get("sample"), 200)})
    for k in ("gather_GBps", "hbm_copy_GBps", "per_step_ms_device_median", "host_enqueue_ms_per_step_median",
              "step_algorithmic_GB", "step_algorithmic_GBps", "allreduce_ms", "exposed_ms"):
        if res.get(k) is not None:
            line[k] = res[k]
    kern = res.get("kernels") or {}
    top = sorted(kern.items(), key=lambda kv: -kv[1]["avg_ms"] * kv[1].get("launches_per_step", 1))[:8]
    line["kernels_ms_per_step"] = {n: v["avg_ms"] * v.get("launches_per_step", 1) for n, v in top}
    if res.get("workloads"):
        line["workloads_ms"] = {n: _workload_ms(w) for n, w in res["workloads"].items()}
    mb = res.get("mapping_build")
    if mb and "images_per_s" in mb:
        line["mapping_build_images_per_s"] = mb["images_per_s"]
    col = res.get("collective")
    if col:
        line["collective"] = {k: col[k] for k in ("per_rank_ms_per_step", "ranks_devices") if k in col}
    line["detail_file"] = detail_file
    line = _sig(line)
    # the cap is a property of the record, not of luck: optional keys go first if a future field overgrows it
    for k in ("collective", "workloads_ms", "kernels_ms_per_step", "host_enqueue_ms_per_step_median",
              "step_algorithmic_GBps"):
        if len(json.dumps(line)) < LINE_TARGET + 2048:
            break
        line.pop(k, None)
    assert len(json.dumps(line)) < LINE_HARD_CAP, "bench line over the driver's 8 KB stdout tail"
    return line


def emit(res, json_fd, detail_file=None):
    """Full record -> bench_detail.json (repo root, and gpurun_out/ when it exists so that it travels back from the GPU
    box; or --detail-file); compact record -> the one stdout line."""
    paths = [detail_file] if detail_file else [os.path.join(d, DETAIL_FILE) for d in (ROOT, os.path.join(ROOT, "gpurun_out"))
                                               if os.path.isdir(d)]
    for p in paths:
        try:
            with open(p, "w") as f:
                json.dump(res, f)
        except OSError as e:
            print(f"bench.py: could not write {p}: {e}", file=sys.stderr)
    os.write(json_fd, (json.dumps(compact_line(res, os.path.basename(paths[0]) if paths else DETAIL_FILE)) + "\n").encode())


DUMP_BUDGET_BYTES = 64 << 20     # --dump-outputs: all files together
DUMP_SAMPLE_BYTES = 24 << 20     # per sampled array (fused features, feature-map gradient)
DUMP_SEED = 20240601


def dump_outputs(out_dir, fused, x, view_pool):
    """--dump-outputs DIR: what the last timed step handed its caller, as float32 .npy files, so that two builds can be
    compared output for output on identical inputs (the scene, the module weights and the upstream gradient are seeded).
      fused.npy               rows of the fused features [N, 4 + C] (all rows if they fit DUMP_SAMPLE_BYTES, else a fixed
                              seeded sample of rows in ascending order)
      x_grad.npy              gradient of the feature maps, flattened in logical [B, C, H, W] order (all of it or a fixed
                              seeded sample of elements in ascending order)
      grad_<parameter>.npy    gradient of every parameter of the view pooling module (whole)
    Returns {name: shape}."""
    os.makedirs(out_dir, exist_ok=True)
    g = torch.Generator().manual_seed(DUMP_SEED)
    arrays = {}
    n, cols = fused.shape
    k = min(n, max(1, DUMP_SAMPLE_BYTES // (4 * cols)))
    rows = torch.arange(n) if k == n else torch.randperm(n, generator=g)[:k].sort()[0]
    arrays["fused"] = fused.detach()[rows.to(fused.device)].float()
    if x.grad is not None:
        gx = x.grad.detach().float().reshape(-1)
        k = min(gx.numel(), DUMP_SAMPLE_BYTES // 4)
        idx = torch.arange(gx.numel()) if k == gx.numel() else torch.randperm(gx.numel(), generator=g)[:k].sort()[0]
        arrays["x_grad"] = gx[idx.to(gx.device)]
    for name, p in view_pool.named_parameters():
        if p.grad is not None:
            arrays["grad_" + name.replace(".", "_")] = p.grad.detach().float()
    arrays = {name: a.cpu().numpy() for name, a in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_BUDGET_BYTES:
        raise SystemExit(f"bench.py: --dump-outputs would write {total} bytes (> {DUMP_BUDGET_BYTES})")
    import numpy as np
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}


def dry_run(args, world, rank, local_rank, json_fd):
    """Hidden `--dry-run` (tests/test_bench_launcher.py): everything bench.py does to become N ranks -- launcher,
    rendezvous, process group, rank / device census, the gradient bucket's all-reduce, max-over-ranks timing -- with
    no HIP work, so that the N > 1 entry is exercised on a box without GPUs (`--backend gloo`)."""
    from deepviewagg_amd.parallel import GradientBucket
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(args.backend, rank=rank, world_size=world)
    device = torch.device("cpu")
    ranks_devices = rank_census(world, rank, local_rank, device, args.backend)
    p = torch.nn.Parameter(torch.zeros(1000))
    p.grad = torch.full((1000,), float(rank + 1))
    bucket = GradientBucket([p])
    t0 = time.perf_counter()
    for _ in range(args.steps):
        bucket.reduce(average=False)
    tt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    if rank == 0:
        res = {"metric": "points/sec fused fwd+bwd (1M pts, 32 views)", "value": None, "unit": "points/s",
               "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "dry_run": True, "backend": args.backend,
               "collective": {"ranks_devices": ranks_devices},
               "allreduce_sum_check": float(p.grad[0].item())}
        os.write(json_fd, (json.dumps(res) + "\n").encode())
    dist.barrier()
    dist.destroy_process_group()


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))
    # stdout carries exactly ONE JSON line: everything else that may write to fd 1 (RCCL prints a version
    # banner there at communicator creation) is redirected to stderr for the duration of the run
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # --gpus is the contract: the process group this rank sits in must have exactly that many ranks
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch with "
                         f"`python bench.py --gpus N` (spawns the ranks itself) or torch.distributed.run "
                         f"--nproc-per-node N ... bench.py --gpus N")
    if args.dry_run:
        return dry_run(args, world, rank, local_rank, json_fd)
    if args.backend != "nccl":
        raise SystemExit("bench.py: --backend gloo exists only for --dry-run; the measured path is RCCL")
    n_dev = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if n_dev <= local_rank:
        raise SystemExit(f"bench.py: rank {rank} of {world} (LOCAL_RANK {local_rank}) has no HIP device: "
                         f"{n_dev} visible, --gpus {args.gpus} needs one per rank")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    # one process per GPU over RCCL; a 1-rank torchrun launch (RANK set) also goes through the process group so
    # that the collective path can be exercised on a single-GPU box
    use_dist = world > 1 or ("RANK" in os.environ and "MASTER_PORT" in os.environ)
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        # RCCL really spans `world` ranks, one per device: all-gather of (rank, device ordinal) -- checked in-process
        ranks_devices = rank_census(world, rank, local_rank, device, "nccl")
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32

    from deepviewagg_amd import ops, _lib
    _lib.load()  # fail loudly if the HIP library is missing

    N, views, C, H, W = 1 << args.log2_points, args.views, args.channels, 64, 128
    if args.strong:
        # the same scene on every rank (same seed), each rank keeps its tile
        scene = tile_of_scene(make_scene(N, views, 32, C, H, W, dtype, device, seed=1234, workload=args.workload),
                              rank, world)
    else:
        scene = make_scene(N, views, 32, C, H, W, dtype, device, seed=1234 + rank, workload=args.workload,
                           upscale=8 if args.interpolate else 1)
    V_scene = int(scene["x_map"].shape[0])
    N_rank = int(scene["csr"].shape[0] - 1)
    mods = build_modules(C, device, args.out_channels)
    from deepviewagg_amd.parallel import GradientBucket
    bucket = GradientBucket(mods[1].parameters())
    # stand-in for the gradients of the model parts outside the path (2D encoder, 3D backbone): all-reduced on a
    # side stream, started when the backward of the path starts, awaited at the end of the step
    standin = None
    if use_dist and args.standin_mb > 0 and not args.no_standin:
        n_el = int(args.standin_mb * 1e6 / 4)
        sp = torch.nn.Parameter(torch.zeros(n_el, device=device))
        sp.grad = torch.full((n_el,), 1e-3, device=device)
        standin = GradientBucket([sp], bucket_bytes=32 << 20)

    def barrier():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    def one_step():
        fused = step(scene, None, mods, dtype, lazy=not args.materialize, interpolate=args.interpolate,
                     before_backward=(lambda: standin.start(average=True)) if standin is not None else None)
        bucket.reduce(average=True)
        if standin is not None:
            standin.finish()
        return fused

    for _ in range(args.warmup + 3):       # + 3: clock ramp / allocator growth of a fresh process, whatever W is
        one_step()
    # per-kernel table: PROFILE_STEPS more UNTIMED steps with HIP events around every launch.  The timed region below
    # carries events only around the kernels its roofline objects report on (the dominant kernel found here and the fused
    # view kernel): a pair of events costs the stream ~6 us of bubble per launch -- 43 pairs = 0.27 ms of an 11.2 ms step
    # in the rocprofv3 trace (profiles/r05b_S1_last_step.txt) -- which is measurement, not the path's work.  A plain run
    # (no --full) takes these steps too: they pick the two kernels the timed region carries events around
    ops.TIMER = ops.KernelTimer()
    for _ in range(PROFILE_STEPS):
        one_step()
    prof_timer, ops.TIMER = ops.TIMER, None
    kern = prof_timer.summary()
    dom_name = max(kern.items(), key=lambda kv: kv[1]["ms"])[0]
    target_name = "chain_attn_fwd" if "chain_attn_fwd" in kern else "view_gather_attention_fwd"
    # A one-off host stall inside the timed region (one step of 47 ms among nineteen of 11.2 ms, twice in six runs on the
    # GPU box) is the host, not the path: the collector of Python cycles is switched off for the K timed steps (a full
    # collection over the module / autograd objects takes tens of ms), and the caching allocator's device allocations
    # during the region are counted and reported.  Two settle steps in the same regime first: the step right after a
    # collection was seen 1.4 ms slow with one device allocation (freed cycles change the allocator's block pattern).
    import gc
    gc.collect()
    gc.disable()
    for _ in range(2):
        one_step()
    barrier()
    ops.TIMER = ops.KernelTimer(only={dom_name, target_name})
    mem0 = torch.cuda.memory_stats(device)
    # one event per step boundary (6 us per step): the device-side duration of every timed step goes into the JSON line,
    # so that a one-off stall (a 33 ms hiccup was seen once in twenty runs) is visible next to the wall-clock value
    marks, host = [], []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append(ev)
        host.append(time.perf_counter())
        fused = one_step()
    end_mark = torch.cuda.Event(enable_timing=True)
    end_mark.record()
    marks.append(end_mark)
    host.append(time.perf_counter())
    barrier()
    elapsed = time.perf_counter() - t0
    gc.enable()
    mem1 = torch.cuda.memory_stats(device)
    alloc_in_region = {k: int(mem1.get(k, 0) - mem0.get(k, 0)) for k in
                       ("num_device_alloc", "num_device_free", "num_alloc_retries", "num_ooms")}
    timer, ops.TIMER = ops.TIMER, None
    dumped = None
    if args.dump_outputs and rank == 0:
        # outside the timed region, before the secondary workloads release the scene
        dumped = dump_outputs(args.dump_outputs, fused, scene["x"], mods[1])
    per_step_device_ms = [a.elapsed_time(b) for a, b in zip(marks[:-1], marks[1:])]
    per_step_host_ms = [(b - a) * 1e3 for a, b in zip(host[:-1], host[1:])]
    collective = None
    if use_dist:
        # what the collectives of the LAST step cost: duration on the side stream, and the part the main stream had to
        # wait for in finish() (0 = fully hidden under the backward)
        t_standin = standin.timings() if standin is not None else None
        t_pool = bucket.timings()
        mine = torch.tensor([elapsed / args.steps * 1e3,
                             t_standin[0] if t_standin else 0.0, t_standin[1] if t_standin else 0.0,
                             t_pool[0] if t_pool else 0.0, t_pool[1] if t_pool else 0.0],
                            device=device, dtype=torch.float64)
        per_rank = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(per_rank, mine)
        per_rank = torch.stack(per_rank).cpu()
        collective = {"per_rank_ms_per_step": [float(v) for v in per_rank[:, 0]],
                      "standin_allreduce_ms": [float(v) for v in per_rank[:, 1]],
                      "standin_exposed_ms": [float(v) for v in per_rank[:, 2]],
                      "pooling_bucket_allreduce_ms": [float(v) for v in per_rank[:, 3]],
                      "pooling_bucket_exposed_ms": [float(v) for v in per_rank[:, 4]],
                      "ranks_devices": ranks_devices,
                      "note": "last timed step; allreduce_ms = copy-in + RCCL all-reduce on the side stream (HIP events), "
                              "exposed_ms = how long the main stream was blocked in finish() waiting for it"}
        tt = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())

    if rank == 0:
        kern_timed = timer.summary()
        ms_per_step = elapsed / args.steps * 1e3
        total_points = N if args.strong else N * world
        value = total_points * args.steps / elapsed
        es = 2 if dtype == torch.bfloat16 else 4
        # dominant HIP kernel of the path: the one with the largest total time per step (profile steps); its launch
        # duration = HIP events around its launches INSIDE the timed region
        name = dom_name
        k = kern_timed.get(name) or kern[name]
        avg_ms = k["ms"] / k["launches"]
        achieved = (k["bytes"] / k["launches"]) / (avg_ms * 1e-3) / 1e9
        default_workload = (args.log2_points == 20 and args.dtype == "bf16" and args.workload == "S1"
                            and args.channels == 64 and args.views == 32 and not args.materialize
                            and not args.strong and not args.interpolate and args.out_channels is None)
        if not args.full:
            _LIVE_PMC["why"] = "run with --full only"
        elif default_workload and world == 1 and not args.no_pmc:
            live_pmc_passes()
        traffic, traffic_why = pmc_traffic(name, default_workload)
        chain = "chain_attn_fwd" in kern
        res = {
            "metric": "points/sec fused fwd+bwd (1M pts, 32 views)",
            "value": value, "unit": "points/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "strong" if args.strong else "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"{args.workload}/F-S: N=2^{args.log2_points} points x "
                                   f"{views if args.workload != 'S2' else 'ragged <= ' + str(views)} views (V={V_scene}"
                                   f"{' on this rank' if args.strong else ''}), "
                                   f"32 feature maps [{C},{H},{W}] {args.dtype} channels-last, "
                                   + ("bilinear gather (mapping at 8x the map resolution), E_mod "
                                      f"{C}->{args.out_channels or C} per view -> " if args.interpolate else "nearest gather -> ")
                                   + f"max atomic pool -> GroupBimodalCSRPool(G=4, DeepSetFeat, train) -> concat; backward seeded "
                                   f"with a fixed upstream gradient [N, 4+C]; "
                                   + ("one scene split into WORLD_SIZE spatial tiles" if args.strong else "one scene per GPU"),
                       "points_per_gpu": N_rank, "views_per_point": views, "parallelism": f"dp{world}",
                       "gradient_allreduce": None if not use_dist else
                       {"pooling_parameters_bytes": int(bucket.flat.numel() * 4),
                        "standin_bucket_MB": args.standin_mb if standin is not None else 0,
                        "note": "stand-in fp32 bucket = the 28.1 M parameters of the full model outside the path "
                                "(SURVEY.md 8(e)); all-reduced (RCCL) on a side stream under the backward of every step"}},
            "roofline": {"bound": "hbm", "kernel": name, "achieved": achieved, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                         "traffic_source": traffic_why if traffic is None else
                         ("measured in this run: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE child passes (1 step), "
                          "FETCH_SIZE x2 (gfx950)" if traffic_why == "live" else
                          "profiles/pmc_traffic_latest.json (stamp = sha256 of the kernel sources, checked against this "
                          "build; live passes: " + str(_LIVE_PMC["why"]) + ")"),
                         "avg_launch_ms": avg_ms, "launches": k["launches"],
                         "algorithmic_bytes_per_launch": k["bytes"] / k["launches"],
                         "note": ROOFLINE_NOTES.get(name, ROOFLINE_NOTES["*"]) if chain else None},
            "kernels": {n: {"avg_ms": v["ms"] / v["launches"], "launches_per_step": v["launches"] / PROFILE_STEPS,
                            "GBps": (v["bytes"] / v["launches"]) / (v["ms"] / v["launches"] * 1e-3) / 1e9}
                        for n, v in sorted(kern.items(), key=lambda kv: -kv[1]["ms"])},
            "kernels_source": f"{PROFILE_STEPS} untimed steps after the warm-up with HIP events around every launch; the "
                              f"timed region times only '{dom_name}' and '{target_name}' (an event pair costs ~6 us of "
                              "stream bubble per launch)",
            "per_step_ms_device": [round(v, 3) for v in per_step_device_ms],
            "per_step_ms_device_median": sorted(per_step_device_ms)[len(per_step_device_ms) // 2],
            "host_enqueue_ms_per_step_median": sorted(per_step_host_ms)[len(per_step_host_ms) // 2],
            "host_enqueue_ms_per_step_max": max(per_step_host_ms),
            "allocator_in_timed_region": alloc_in_region,
            "step_algorithmic_GB": sum(v["bytes"] for v in kern.values()) / PROFILE_STEPS / 1e9,
            "hbm_copy_GBps": None,
            "gather_GBps": None,
            "fused_abs_mean": float(fused.float().abs().mean().item()),
        }
        res["step_algorithmic_GBps"] = res["step_algorithmic_GB"] / (ms_per_step * 1e-3)
        if dumped is not None:
            res["dump_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
        if _LIVE_PMC["table"] is not None:
            res["pmc_live"] = {"calibration_on_copy_kernel": _LIVE_PMC["table"].get("_calibration"),
                               "hbm_bytes_per_launch": {t: (_pmc_lookup(_LIVE_PMC["table"], t) or {}).get("hbm_bytes")
                                                        for t in KERNEL_SYMBOL}}
        else:
            res["pmc_live"] = {"skipped": _LIVE_PMC["why"]}
        if collective is not None:
            res["allreduce_ms"] = max(collective["standin_allreduce_ms"])
            res["exposed_ms"] = max(a + b for a, b in zip(collective["standin_exposed_ms"],
                                                          collective["pooling_bucket_exposed_ms"]))
            res["collective"] = collective
        if args.full:
            # practical ceiling next to the nominal one: the float4 copy kernel in this process
            res["hbm_copy_GBps"] = copy_ceiling(device)
            res["roofline"]["copy_ceiling"] = res["hbm_copy_GBps"]
            res["roofline"]["frac_of_copy_ceiling"] = achieved / res["hbm_copy_GBps"]
        # the kernel the north star's >= 70 % target names: the fused view-gather + attention forward
        tname = target_name
        tk = kern_timed.get(tname) or kern.get(tname)
        if tk is not None:
            t_ms = tk["ms"] / tk["launches"]
            nb = fused_fwd_bytes(V_scene, N_rank, C, es) if chain else tk["bytes"] / tk["launches"]
            t_ach = nb / (t_ms * 1e-3) / 1e9
            res["roofline_view_gather_attention"] = {
                "bound": "hbm", "kernel": tname, "achieved": t_ach, "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": t_ach / HBM_PEAK_GBS, "avg_launch_ms": t_ms, "launches": tk["launches"],
                "algorithmic_bytes_per_launch": nb,
                "traffic": pmc_traffic(tname, default_workload)[0],
                "note": "x_map + value rows in -> pooled features out in ONE kernel (DeepSetFeat scores, softmax, row "
                        "gather, weighted sum, gate); SURVEY.md 8(d) bytes V (C s + 32 + 8) + N (C s + 8), every "
                        "gathered row counted as an HBM read although the rows of this workload come out of a 33 MB "
                        "map (cache hierarchy); the kernel also reads 128 bytes per point (set-branch row)"}
            if res["hbm_copy_GBps"] is not None:
                res["roofline_view_gather_attention"]["frac_of_copy_ceiling"] = t_ach / res["hbm_copy_GBps"]
        # everything below is --full only: measurements of their own, none of them needed by the headline
        if args.full and world == 1 and not args.no_mapping_build:
            # M2: the materialised nearest gather at the scene's V (outside the step timer)
            g = gather_bench(scene)
            res["gather_GBps"] = g["GBps"]
            res["gather"] = g
            res["mapping_build"] = mapping_build_bench(device)
            res["neighborhood_features"] = neighborhood_bench(device)
        if args.full and world == 1 and not args.no_secondary and default_workload:
            del scene
            torch.cuda.empty_cache()
            res["workloads"] = {
                "S2": secondary_workload("S2", device, dtype, args.log2_points, views, 64),
                "F-L": secondary_workload("F-L", device, dtype, args.log2_points, views, 512),
                "S1c": secondary_workload("S1c", device, dtype, args.log2_points, views, 64),
                # interpolate=True (the published KITTI-360 configuration): C = 64 and the KITTI pair l0 128 -> 32
                "bilinear_C64": secondary_workload("bilinear", device, dtype, args.log2_points, views, 64,
                                                   interpolate=True),
                "bilinear_kitti_128_32": secondary_workload("bilinear", device, dtype, args.log2_points, views, 128,
                                                            interpolate=True, C_out=32),
                # the reference's default arithmetic (no autocast, fp32 features): S1 shapes on the fp32 chain
                "f32": secondary_workload("f32", device, torch.float32, args.log2_points, views, 64),
                "kitti360_pyramid_eval": kitti360_pyramid_eval(device, args.log2_points, views),
                # QKVBimodalCSRPool (pooling.py:454-547) at the S1 shapes: keys = one more layer of the recompute chain (round 4)
                "qkv": secondary_workload("qkv", device, dtype, args.log2_points, views, 64),
                "kitti360_pyramid_train": kitti360_pyramid_train(device, args.log2_points, views),
                "s3dis_batch": s3dis_batch_workload(device),
                "nonexact": nonexact_workload(device),
                # a multi-setting batch (two map sizes) on the fused bilinear path (round 6)
                "bilinear_two_settings": two_setting_bilinear_workload(device, args.log2_points, views),
            }
        if args.full and world == 1 and not args.no_cpu_baseline:
            # cpu_baseline.value = the build's own C + OpenMP restatement of the WHOLE step on all host
            # cores; the PyTorch-CPU op sequence (dispatch-bound, effectively one core) and the
            # gather + attention-only twin are sub-keys
            threads = min(os.cpu_count() or 1, 64)
            mem = _host_mem_available_gb()
            log2_cpu = min(args.log2_points, 20 if mem > 200 else 19 if mem > 100 else 18 if mem > 40 else 16)
            try:
                res["cpu_baseline"] = cpu_full_path_twin(log2_cpu, views, C)
                res["cpu_baseline"]["host"] = {"os_cpu_count": os.cpu_count(), "mem_available_GB": mem,
                                               "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS")}
                res["cpu_baseline"]["gather_attention_openmp_twin"] = cpu_gather_attention_twin(
                    min(args.log2_points, 18), views, C)
            except OSError as e:         # the oracle library is built by __graft_entry__.build()
                res["cpu_baseline"] = {"error": str(e)}
            res["cpu_baseline"]["pytorch_oracle"] = cpu_baseline(args.cpu_log2_points, views, C, threads)
        emit(res, json_fd, args.detail_file)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
