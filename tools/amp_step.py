"""bf16 against fp16 autocast on the S1 headline step (2^20 points x 32 views, C = 64, G = 4, train, forward + backward,
mapping rebuilt every step), in one process: the two arms alternate step by step, each timed with HIP events.

    python tools/amp_step.py [--log2-points 20] [--warmup 5] [--steps 20] [--out profiles/amp_step_fp16.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/amp_step.py --arms fp16   (one traced run per arm, then)
    python tools/amp_step.py --out profiles/amp_step_fp16.json --merge-stats BF16_STATS.csv FP16_STATS.csv

The step is bench.step's dataflow (lazy nearest gather -> atomic max pool -> GroupBimodalCSRPool -> fusion concat,
backward seeded with a fixed upstream gradient) with the autocast dtype as a parameter; the map is stored in the
autocast dtype."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def run_step(scene, mods, dtype):
    from deepviewagg_amd import ops
    atomic_pool, view_pool, fusion = mods
    x = scene["x"].requires_grad_(True)
    x.grad = None
    for p in view_pool.parameters():
        p.grad = None
    with torch.autocast("cuda", dtype=dtype):
        x_mod = ops.lazy_gather_nearest_mapping(x, scene["images"], scene["atom_ptr"], scene["pixels"], 1.0, exact=True)
        x_mod = atomic_pool(None, x_mod, None, scene["atom_ptr"])
        x_pool = view_pool(scene["x_3d"], x_mod, scene["x_map"], scene["csr"])
        out = fusion(scene["x_3d"], x_pool)
    if scene.get("grad_out") is None:
        scene["grad_out"] = torch.randn(out.shape, device=out.device, dtype=out.dtype,
                                        generator=torch.Generator(device=out.device).manual_seed(99)) / out.shape[0]
    out.backward(scene["grad_out"])
    return x_pool.dtype


def count_chain_launches():
    """Counts the view-kernel launches per row dtype (dva_chain_attn_fwd_dt / _bwd_dt): the proof that an arm ran the chain,
    not the generic path (whose pooled output has the same dtype)."""
    from deepviewagg_amd import _lib
    lib = _lib.load()
    counts = {}
    for name in ("dva_chain_attn_fwd_dt", "dva_chain_attn_bwd_dt"):
        orig = getattr(lib, name)

        def f(*a, _orig=orig, _name=name):
            key = f"{_name}:{'fp16' if a[-2] == _lib.DVA_F16 else 'bf16'}"
            counts[key] = counts.get(key, 0) + 1
            return _orig(*a)
        setattr(lib, name, f)
    return counts


KERNELS = ("attn_fwd_kernel", "attn_bwd_kernel", "bucket_rows_grad_kernel")


def kernel_stats(csv_paths):
    """Mean duration (us) of the view kernel, the attention backward and the bucket rows gradient in rocprofv3 --stats files,
    per row type: bf16 = unsigned short (``t`` when the name is left mangled), fp16 = _Float16 (``DF16_``)."""
    import csv
    out = {}
    for path in csv_paths:
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r["Name"]
                base = next((k for k in KERNELS if k in name), None)
                if base is None:
                    continue
                kind = "fp16" if ("_Float16" in name or "DF16_" in name) else "bf16"
                key = f"{base}[{kind}]"
                e = out.setdefault(key, {"calls": 0, "total_us": 0.0})
                e["calls"] += int(r["Calls"])
                e["total_us"] += float(r["TotalDurationNs"]) / 1e3
    for e in out.values():
        e["mean_us"] = e["total_us"] / max(e["calls"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-points", type=int, default=20)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--arms", default="bf16,fp16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge-stats", nargs=2, metavar=("BF16_CSV", "FP16_CSV"), default=None,
                    help="no run: add the kernel means of two rocprofv3 --stats files (one per arm) to --out")
    args = ap.parse_args()
    if args.merge_stats:
        with open(args.out) as f:
            res = json.load(f)
        arms = {"bf16": kernel_stats([args.merge_stats[0]]), "fp16": kernel_stats([args.merge_stats[1]])}
        res["kernels_mean_us"] = {arm: {k: round(v["mean_us"], 2) for k, v in st.items()} for arm, st in arms.items()}
        with open(args.out, "w") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps(res["kernels_mean_us"]))
        return
    if not torch.cuda.is_available():
        raise SystemExit("amp_step.py measures on a HIP device; none is visible")
    dev = "cuda:0"
    N, C = 1 << args.log2_points, args.channels
    dtypes = {"bf16": torch.bfloat16, "fp16": torch.float16}
    arms = {}
    for name in args.arms.split(","):
        dt = dtypes[name]
        scene = bench.make_scene(N, args.views, 32, C, 64, 128, dt, dev, seed=4321)
        arms[name] = (scene, bench.build_modules(C, dev), dt)
    launches = count_chain_launches()
    times = {name: [] for name in arms}
    pooled = {}
    for i in range(args.warmup + args.steps):
        for name, (scene, mods, dt) in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            pooled[name] = str(run_step(scene, mods, dt))
            b.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name].append(a.elapsed_time(b))
    res = {"workload": "S1", "points": N, "views_per_point": args.views, "channels": C, "groups": 4,
           "warmup": args.warmup, "steps": args.steps, "device": torch.cuda.get_device_name(0),
           "arms": {name: {"pooled_dtype": pooled[name], "ms_median": statistics.median(t), "ms_min": min(t),
                           "ms_max": max(t)} for name, t in times.items()}}
    res["chain_launches"] = launches
    for name in arms:                  # every timed step of every arm went through the chain's view kernels
        assert launches.get(f"dva_chain_attn_fwd_dt:{name}", 0) >= args.warmup + args.steps, launches
    if "bf16" in times and "fp16" in times:
        res["fp16_over_bf16"] = res["arms"]["fp16"]["ms_median"] / res["arms"]["bf16"]["ms_median"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
