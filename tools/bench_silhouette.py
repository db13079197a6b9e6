"""Times acav_rows_silhouette -- the exact silhouette of a labelled sample, every pairwise distance in float64 on the f64 matrix
core -- at the sizes `evaluate --evaluate.silhouette_sample` is run at: Gaussian-mixture rows on the device, labels = the
mixture component.

    python tools/bench_silhouette.py [--m 8192,32768] [--d 128,1024] [--k 256,1024] [--repeat 7] [--out profiles/silhouette_1gpu.json]

Prints one JSON line:
  mfma_f64_tflops     what a bare loop of v_mfma_f64_16x16x4_f64 reaches (tools/exp/mfma_f64_rate.hip, run as a child process
                      before this one opens the device; null when it can be neither found nor built)
  per shape "m:d:k":
    ms                median wall time of a call, which returns when row_stats [m][2] is on the device (a host clock around a call
                      that ends in a stream synchronise); the call includes the label check, the host's stable sort of the
                      positions, the norms and the sweep
    ms_min, ms_max    the spread of the timed calls
    tflops            2 m^2 d / ms: the multiply-adds of the dots (both triangles are computed: a row needs its own sums), two
                      flops each
    of_mfma           tflops / mfma_f64_tflops
    plan              acav_rows_silhouette_plan for this device
    silhouette        the mean s of the call (what the figure is for; the same value every call)
Every shape is warmed up with two calls first; medians of --repeat calls."""
import argparse
import ctypes as C
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
    ap.add_argument("--m", default="8192,32768")
    ap.add_argument("--d", default="128,1024")
    ap.add_argument("--k", default="256,1024")
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rate64 = mfma_f64_tflops()  # before this process opens the device: one program at a time on the matrix cores
    import numpy as np
    import torch
    import acav100m_amd
    acav100m_amd.configure_runtime(quiet=True)
    from acav100m_amd import _lib
    lib = _lib.load_library()
    cus = C.c_int(0)
    _lib.check(lib.acav_device_info(0, None, 0, C.byref(cus), None))
    row = {"repeat": args.repeat, "cus": cus.value, "mfma_f64_tflops": rate64, "shapes": {}}
    for m in (int(v) for v in args.m.split(",")):
        for d in (int(v) for v in args.d.split(",")):
            for k in (int(v) for v in args.k.split(",")):
                gen = torch.Generator(device="cuda").manual_seed(7)
                labels = torch.randint(0, k, (m,), device="cuda", generator=gen)
                centres = torch.randn(k, d, device="cuda", generator=gen)
                x = (centres[labels] + 0.6 * torch.randn(m, d, device="cuda", generator=gen)).contiguous()
                stats = torch.empty(m, 2, dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()

                def call():
                    _lib.check(lib.acav_rows_silhouette(0, _lib.ptr(x), m, d, _lib.ptr(labels), k, _lib.ptr(stats), None))
                for _ in range(2):
                    call()
                times = []
                for _ in range(args.repeat):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    call()  # returns after its stream synchronise
                    times.append((time.perf_counter() - t0) * 1e3)
                ms = statistics.median(times)
                plan = (C.c_int64 * 9)()
                _lib.check(lib.acav_rows_silhouette_plan(m, d, k, cus.value, plan))
                A, B = stats[:, 0].cpu().numpy(), stats[:, 1].cpu().numpy()
                tflops = 2.0 * m * m * d / ms / 1e9
                row["shapes"]["{}:{}:{}".format(m, d, k)] = {
                    "ms": ms, "ms_min": min(times), "ms_max": max(times), "tflops": tflops,
                    "of_mfma": (tflops / rate64) if rate64 else None, "plan": [int(v) for v in plan],
                    "silhouette": float(np.mean((B - A) / np.maximum(A, B)))}
                print("m {:>6} d {:>5} k {:>5}: {:9.3f} ms  {:7.2f} Tflop/s".format(m, d, k, ms, tflops), file=sys.stderr, flush=True)
                del x, stats, labels, centres
                torch.cuda.empty_cache()
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
