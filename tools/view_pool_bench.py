#!/usr/bin/env python
"""Time the view-level ``BimodalCSRPool`` (mean by default) on lazily gathered features: the fused route against the
materialised route (``x_mod.materialize()`` + ``ops.segment_csr``) on the same build and device.

--gather nearest: ``ops.gather_segment_reduce`` (csrc/gather_reduce.hip, all four modes) against
``ops.LAZY_REDUCE = False`` (max: ``ops.LAZY_NONEXACT = False``, the switch of the max pool).  --gather bilinear: ``ops.interp_segment_reduce``
(csrc/interp_reduce.hip) against ``ops.LAZY_INTERP_REDUCE = False`` on the same scenes, the views' coordinates being their
pixels over the mapping size as ``bench.py`` forms them.

Scenes are ``bench.make_scene`` at the benchmark's view distribution (S1: 32 views per point over 32 images of 64 x 128
map rows; S2 with --workload S2), N = 3 x 10^5 and 2^20 points, C = 13 / 64 / 128, bf16 and fp32 maps.  One measurement
is forward + backward of the pool (the output gradient handed in), timed with device events; the two routes alternate
in one process after --warmup untimed rounds, and the table holds the median and [min, max] over --reps.  ``launches``
are the device kernels of one forward + backward as the torch profiler counts them in a separate, untimed pass (None
where the profiler is not available), ``peak_bytes`` the peak of allocated device memory above the inputs in one more
untimed pass, ``hbm_share`` the algorithmic bytes of the fused kernels over the median time, as a fraction of the
8 TB/s HBM specification -- for both routes, so it is each route's rate on the same bytes.  Algorithmic bytes, what the
pool has to move, with P items, S segments, R map rows, C channels of s bytes:
  nearest   forward P (4 + C s) + S (8 + C s), backward P (16 + C s) + R (4 + C s) for the mean (sum: 8 bytes per item
            less; min / max: 2 S C arg offsets forward, 2 P C backward);
  bilinear  forward P (32 + 4 C s) + S (8 + C s) -- the taps and four map rows per item --, backward
            4 P (12 + C s + 8) + R (4 + C s) for the mean -- per tap its plan entry, weight, the item's segment, the
            segment's bounds and gradient row -- (sum: 8 bytes per tap less; max / min: 2 S C arg offsets forward,
            8 P C backward).  Where the backward runs over the anchor plan (fp32 / bf16, C / (16 / s) a power of two
            <= 64: ``ops._anchor_ok``) it is P (24 + C s + 16) + A (4 + 32 C) + R C (4 + s) with A anchors: per item
            its plan entry, four weights, segment, bounds and gradient row ONCE, the fp32 per-anchor sums written and
            read, the fp32 map gradient written and cast.  The plan (a sort of 4 P tap keys or P anchor keys) is not
            part of these bytes: it is overhead of the route, in its time.  On those shapes a third route,
            ``fused_tap_plan`` (``ops.INTERP_REDUCE_ANCHOR = False``), is timed in the same alternation: the A/B of the
            two backward plans on the same rows (its ``hbm_share`` is on the tap plan's own bytes).
The outputs of the two routes are compared bit for bit, the gradients by their largest difference.  One JSON line on
stdout; --out writes it (profiles/view_pool_bench.json, profiles/view_pool_bilinear_bench.json).

Usage:  python tools/view_pool_bench.py [--gather nearest] [--reps 7] [--warmup 2] [--mode mean ...] [--workload S1]
                                        [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import measure  # noqa: E402

POINTS = (300000, 1 << 20)
CHANNELS = (13, 64, 128)
DTYPES = (torch.bfloat16, torch.float32)
VIEWS, IMAGES, H, W = 32, 32, 64, 128
HBM_SPEC_BYTES_PER_S = 8.0e12


def algorithmic_bytes(P, S, R, C, es, mode, gather="nearest", anchors=None):
    arg = mode in ("min", "max")
    if gather == "bilinear":
        fwd = P * (32 + 4 * C * es) + S * (8 + C * es) + (2 * S * C if arg else 0)
        if anchors is not None:      # the anchor plan: per item its plan entry, weights, segment, bounds and gradient row
            bwd = P * (24 + C * es + (0 if mode == "sum" else 16) + (2 * C if arg else 0)) + anchors * (4 + 32 * C) \
                + R * C * (4 + es)
        else:
            bwd = 4 * P * (12 + C * es + (0 if mode == "sum" else 8) + (2 * C if arg else 0)) + R * (4 + C * es)
        return fwd + bwd
    fwd = P * (4 + C * es) + S * (8 + C * es) + (2 * S * C if arg else 0)
    bwd = P * (8 + C * es + (0 if mode == "sum" else 8) + (2 * C if arg else 0)) + R * (4 + C * es)
    return fwd + bwd


def run_case(bench, n, C, dtype, mode, workload, reps, warmup, gather="nearest"):
    from deepviewagg_amd import ops
    from deepviewagg_amd.modules.multimodal import pooling as P
    dev = torch.device("cuda", 0)
    scene = bench.make_scene(n, VIEWS, IMAGES, C, H, W, dtype, dev, seed=4321, workload=workload)
    x = scene["x"].requires_grad_()
    csr, x_map = scene["csr"], scene["x_map"]
    if gather == "bilinear":
        packed = ops.pack_gather_index(scene["images"], scene["atom_ptr"], scene["pixels"], ratio=1.0)
        size = torch.tensor([scene["mapping_size"]], dtype=torch.float32, device=dev)
        feats = ops.lazy_gather_bilinear(x, packed, (scene["pixels"] / (size - 1))[:, [1, 0]], exact=True)
        switch = "LAZY_INTERP_REDUCE"
    else:
        feats = ops.lazy_gather_nearest_mapping(x, scene["images"], scene["atom_ptr"], scene["pixels"], 1.0, exact=True)
        switch = "LAZY_NONEXACT" if mode == "max" else "LAZY_REDUCE"
    V, S, R = feats.shape[0], csr.shape[0] - 1, feats.rows.shape[0]
    w = torch.randn(S, C, device=dev).to(dtype)
    pool = P.BimodalCSRPool(mode=mode)

    def step(fused):
        setattr(ops, switch, fused)
        try:
            out = pool(None, feats, x_map, csr)
            (g,) = torch.autograd.grad(out, x, grad_outputs=w)
        finally:
            setattr(ops, switch, True)
        return out, g

    def step_tap_plan():
        ops.INTERP_REDUCE_ANCHOR = False
        try:
            return step(True)
        finally:
            ops.INTERP_REDUCE_ANCHOR = True

    routes = {"fused": lambda: step(True), "materialised": lambda: step(False)}
    anchored = gather == "bilinear" and ops._anchor_ok(C, dtype)
    if anchored:
        routes["fused_tap_plan"] = step_tap_plan
    (out_f, g_f), (out_m, g_m) = routes["fused"](), routes["materialised"]()
    agree = {"out_equal": bool(torch.equal(out_f, out_m)),
             "grad_max_abs_diff": float((g_f.float() - g_m.float()).abs().max()),
             "grad_max_abs": float(g_m.float().abs().max())}
    del out_f, g_f, out_m, g_m
    # every window starts on an idle device
    ms, _ = measure.alternate(routes, reps, measure.event_window, warmup=warmup,
                              before=lambda key, rep: torch.cuda.synchronize())
    nbytes = algorithmic_bytes(V, S, R, C, x.element_size(), mode, gather,
                               ops.n_anchors(feats.geometry) + 1 if anchored else None)
    tap_bytes = algorithmic_bytes(V, S, R, C, x.element_size(), mode, gather)
    res = {"N": n, "V": V, "map_rows": R, "C": C, "dtype": str(dtype)[6:], "mode": mode, "workload": workload,
           "gather": gather, "plan": type(getattr(feats, "plan", None)).__name__, "algorithmic_bytes": nbytes,
           "backward_plan": ("anchor" if anchored else "tap") if gather == "bilinear" else "row", "agree": agree}
    for k, fn in routes.items():
        t = measure.summarise(ms[k], 4)
        t = {"median_ms": t["median"], "min_ms": t["min"], "max_ms": t["max"]}
        share_of = tap_bytes if k == "fused_tap_plan" else nbytes
        res[k] = dict(t, launches=measure.profiler_kernel_count(fn), peak_bytes=measure.peak_bytes(fn),
                      hbm_share=round(share_of / (t["median_ms"] * 1e-3) / HBM_SPEC_BYTES_PER_S, 4))
    res["speedup"] = round(res["materialised"]["median_ms"] / res["fused"]["median_ms"], 3)
    if anchored:
        res["anchor_over_tap_plan"] = round(res["fused_tap_plan"]["median_ms"] / res["fused"]["median_ms"], 3)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gather", default="nearest", choices=("nearest", "bilinear"))
    ap.add_argument("--mode", nargs="+", default=["mean"], choices=("mean", "sum", "min", "max"))
    ap.add_argument("--workload", default="S1", choices=("S1", "S2"))
    ap.add_argument("--points", type=int, nargs="*", default=list(POINTS))
    ap.add_argument("--channels", type=int, nargs="*", default=list(CHANNELS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "view_pool_bench needs a HIP device"
    import bench
    result = measure.header(
        "view_pool_bench", gather=args.gather, reps=args.reps, warmup=args.warmup,
        timing="device events around forward + backward of BimodalCSRPool on lazily gathered features, the two "
               "routes alternating in one process; median and [min, max] over reps",
        hbm_spec_bytes_per_s=HBM_SPEC_BYTES_PER_S,
        cases=[run_case(bench, n, C, dt, mode, args.workload, args.reps, args.warmup, args.gather)
               for mode in args.mode for n in args.points for C in args.channels for dt in DTYPES])
    result["kernel_sources_sha256"] = result["source_sha256"]               # the name earlier records carry
    measure.emit(result, args.out)


if __name__ == "__main__":
    main()
