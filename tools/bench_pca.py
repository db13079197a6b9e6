"""Times the two sweeps of clustering.pca_dim at the size of real views -- 1M x 1024 -> 256 and 1M x 2304 -> 256, fp32 rows on
the device -- against the roofs they can be held to.

    python tools/bench_pca.py [--n 1000000] [--shapes 1024:256,2304:256] [--repeat 5] [--segments 1,1000] [--out profiles/pca_1gpu.json]

Prints one JSON line:
  copy_GBps               a device-to-device copy of the rows in the same process (reads + writes over the time): the HBM rate
                          this process reaches, the yardstick of the byte roofs
  mfma_f64_tflops         what a bare loop of v_mfma_f64_16x16x4_f64 reaches (tools/exp/mfma_f64_rate.hip, run as a child
                          process; built with hipcc when the program is missing; null when neither is possible)
  per shape "d:p":
    scatter_ms[segments]  acav_rows_scatter into device accumulators: median wall time of a call, which returns when they are up
                          to date, once per segment count (equal segments of n / segments rows)
    scatter_flop_ms       n d (d + 64) flops (the block pairs bi <= bj that are computed, 2 flops a multiply-add) at mfma_f64_tflops
    scatter_read_ms       4 n d bytes at copy_GBps -- a single pass over the rows
    scatter_roof          which of the two is larger, and scatter_of_roof = scatter_ms["1"] over it
    project_ms            acav_rows_project: median wall time of a call
    project_hbm_ms        4 n (d + p) bytes at copy_GBps; project_flop_ms: 2 n d p flops at --f32_tflops (157.3, the fp32 matrix
                          peak of the data sheet: the instruction is exact fp32 at the vector rate); project_roof likewise
Every shape is warmed up with two calls first; medians of --repeat calls."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def mfma_f64_tflops():
    exe, src = os.path.join(ROOT, "tools", "exp", "mfma_f64_rate"), os.path.join(ROOT, "tools", "exp", "mfma_f64_rate.hip")
    try:
        if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
            subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", src, "-o", exe])
        out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
        return json.loads(out.strip().splitlines()[-1])["tflops"]
    except Exception as exc:
        print("the bare MFMA loop did not run: {}".format(exc), file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--shapes", default="1024:256,2304:256")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--segments", default="1,1000")
    ap.add_argument("--f32_tflops", type=float, default=157.3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rate64 = mfma_f64_tflops()  # before this process opens the device: one program at a time on the matrix cores
    import numpy as np
    import torch
    import acav100m_amd
    acav100m_amd.configure_runtime(quiet=True)
    from acav100m_amd import _lib
    from acav100m_amd.clustering import ScatterMoments, project
    lib = _lib.load_library()
    n = args.n
    row = {"n": n, "repeat": args.repeat, "mfma_f64_tflops": rate64, "shapes": {}}

    def median_ms(fn, warm=2):
        for _ in range(warm):
            fn()
        times = []
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(times)

    for shape in args.shapes.split(","):
        d, p = (int(v) for v in shape.split(":"))
        gen = torch.Generator(device="cuda").manual_seed(7)
        x = torch.empty(n, d, device="cuda")
        for s in range(0, n, 65536):
            e = min(n, s + 65536)
            x[s:e] = 0.3 * torch.randn(e - s, d, device="cuda", generator=gen) + 1.0
        nbytes = 4 * n * d
        if "copy_GBps" not in row:
            y = torch.empty_like(x)
            row["copy_GBps"] = 2 * nbytes / median_ms(lambda: y.copy_(x)) / 1e6
            del y
        bw = row["copy_GBps"] * 1e6  # bytes per ms
        res = {"scatter_ms": {}}
        shift = np.ones(d, np.float32)
        for nseg in (int(v) for v in args.segments.split(",")):
            prefix = np.linspace(0, n, nseg + 1).astype(np.int64)
            sm = ScatterMoments(d, shift, "cuda:0")

            def scatter():
                _lib.check(lib.acav_rows_scatter(0, _lib.ptr(x), n, d, _lib.ptr(prefix), nseg, _lib.ptr(shift), _lib.ptr(sm.sum),
                                                 _lib.ptr(sm.scatter), None))
            res["scatter_ms"][str(nseg)] = median_ms(scatter, warm=1)
            del sm
        res["scatter_flop_ms"] = None if not rate64 else n * d * (d + 64.0) / (rate64 * 1e9)
        res["scatter_read_ms"] = nbytes / bw
        roofs = {"flop": res["scatter_flop_ms"] or 0.0, "read": res["scatter_read_ms"]}
        res["scatter_roof"] = max(roofs, key=roofs.get)
        res["scatter_of_roof"] = res["scatter_ms"]["1"] / roofs[res["scatter_roof"]]
        mean = np.ones(d, np.float32)
        comps = (np.random.RandomState(1).randn(p, d) / np.sqrt(d)).astype(np.float32)
        y = torch.empty(n, p, device="cuda")

        def proj():
            _lib.check(lib.acav_rows_project(0, _lib.ptr(x), n, d, _lib.ptr(mean), _lib.ptr(comps), p, _lib.ptr(y), None))
        res["project_ms"] = median_ms(proj)
        res["project_hbm_ms"] = 4.0 * n * (d + p) / bw
        res["project_flop_ms"] = 2.0 * n * d * p / (args.f32_tflops * 1e9)
        roofs = {"flop": res["project_flop_ms"], "hbm": res["project_hbm_ms"]}
        res["project_roof"] = max(roofs, key=roofs.get)
        res["project_of_roof"] = res["project_ms"] / roofs[res["project_roof"]]
        assert tuple(project(x[:64], mean, comps).shape) == (64, p)
        row["shapes"][shape] = res
        del x, y
        torch.cuda.empty_cache()
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
