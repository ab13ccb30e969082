"""Times of the dash stage on a dashed C3: scenes.py's C3 cubics (100 k open cubics, one per path) with the pattern [6, 3].

In one run: the device time of jh_dash (the hipEvent pair of its profile query "dash": the job's upload and the seven kernel
launches), the wall time of the call with the download of index and elements, and the wall time of the host route (jl_dash_path,
one call per path, on a sample of the paths scaled to all of them -- the per-call ctypes overhead is measured on an empty path
and subtracted).  Median of the repetitions.  Writes a JSON file (default profiles/dash_kernel_times.json).  Run on the GPU box:

    python tools/time_dash.py [--paths 100000] [--reps 11] [--host-sample 4000] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import time

import numpy as np

from timing import ROOT, write_json

import jello_amd  # noqa: E402 (timing puts the root on sys.path)
from jello_amd import _lib, scenes  # noqa: E402
from jello_amd.engine import DASH_EL  # noqa: E402

EL = np.dtype([("kind", "<i4"), ("pad", "<i4"), ("pts", "<f8", 6)])      # jh_dash_el
DESC = np.dtype([("first_el", "<u4"), ("n_els", "<u4"), ("first_dash", "<u4"), ("n_dash", "<u4"), ("offset", "<f8")])  # jh_dash_path


def c3_job(n_paths, size=4096, spread=32.0):
    """The control points of scene_c3's cubics as jh_dash's host arrays (the same uniforms in the same order)."""
    u = scenes.splitmix64_array(n_paths * 17, scenes.SEED).reshape(n_paths, 17)
    anchor = u[:, 0:2] * size
    els = np.zeros(2 * n_paths, dtype=EL)
    els["kind"][1::2] = 3
    els["pts"][0::2, 0:2] = anchor
    for k in range(3):
        els["pts"][1::2, 2 * k:2 * k + 2] = anchor + (u[:, 2 + 2 * k:4 + 2 * k] * 2.0 - 1.0) * spread
    desc = np.zeros(n_paths, dtype=DESC)
    desc["first_el"] = 2 * np.arange(n_paths)
    desc["n_els"] = 2
    desc["n_dash"] = 2
    return els, desc, np.array([6.0, 3.0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--host-sample", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dash_kernel_times.json"))
    a = ap.parse_args()
    eng = jello_amd.Engine(0)
    hip, ctx, L = eng.hip, eng.ctx, eng._L
    els, desc, dashes = c3_job(a.paths)
    vp = ctypes.c_void_p
    els_p = ctypes.cast(els.ctypes.data, ctypes.POINTER(_lib.PathEl))
    desc_p = ctypes.cast(desc.ctypes.data, ctypes.POINTER(_lib.CDashPath))
    dash_p = dashes.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ids = (0x7D45_0000_0001, 0x7D45_0000_0002)
    index = np.zeros(a.paths + 1, dtype=np.uint32)
    cap = 16 * a.paths
    eng._check(hip.jh_buffer_create(ctx, ids[1], index.nbytes), "buffer_create")

    def call():
        eng._check(hip.jh_dash(ctx, els_p, len(els), desc_p, a.paths, dash_p, 2, vp(hip.jh_buffer_device_ptr(ctx, ids[0])), cap,
                               vp(hip.jh_buffer_device_ptr(ctx, ids[1]))), "jh_dash")

    for _ in range(2):  # size the element buffer from the reported need, as Engine.dash_paths does
        eng._check(hip.jh_buffer_create(ctx, ids[0], cap * DASH_EL.itemsize), "buffer_create")
        call()
        eng._check(hip.jh_download(ctx, ids[1], index.ctypes.data, 0, index.nbytes), "download")
        cap = max(cap, int(index[-1]))
    total = int(index[-1])
    out_els = np.zeros(total, dtype=DASH_EL)

    device_ms, call_ms = [], []
    for _ in range(a.reps):
        eng.sync()
        eng.profile(True)
        call()
        tree = eng.profile_collect_tree()
        eng.profile(False)
        q = [n for n in tree if n["kind"] == "query" and n["label"] == "dash"]
        device_ms.append(q[0]["gpu_end_ms"] - q[0]["gpu_start_ms"])
        eng.sync()
        t0 = time.perf_counter()
        call()
        eng._check(hip.jh_download(ctx, ids[1], index.ctypes.data, 0, index.nbytes), "download")
        eng._check(hip.jh_download(ctx, ids[0], out_els.ctypes.data, 0, out_els.nbytes), "download")
        call_ms.append((time.perf_counter() - t0) * 1e3)

    # the host route on a sample, byte-compared with the device's elements of the same paths
    n = min(a.host_sample, a.paths)
    out = (_lib.PathEl * 4096)()
    empty = (_lib.PathEl * 1)()
    t0 = time.perf_counter()
    for i in range(n):
        L.jl_dash_path(empty, 0, dash_p, 2, 0.0, out, 4096)
    overhead = time.perf_counter() - t0
    t0 = time.perf_counter()
    counts = [L.jl_dash_path(ctypes.cast(els[2 * i:].ctypes.data, ctypes.POINTER(_lib.PathEl)), 2, dash_p, 2, 0.0, out, 4096) for i in range(n)]
    host_s = time.perf_counter() - t0
    assert counts == [int(index[i + 1] - index[i]) for i in range(n)], "host route and device stage disagree on the element counts"
    r = {"tool": "tools/time_dash.py", "device": eng.device_info()["name"], "paths": a.paths, "pattern": [6.0, 3.0], "elements_out": total,
         "reps": a.reps, "device_ms": round(statistics.median(device_ms), 4), "device_ms_min_max": [round(min(device_ms), 4), round(max(device_ms), 4)],
         "call_and_download_ms": round(statistics.median(call_ms), 3), "call_and_download_ms_min_max": [round(min(call_ms), 3), round(max(call_ms), 3)],
         "host_route_sample": n, "host_route_ms_all_paths": round((host_s - overhead) / n * a.paths * 1e3, 1),
         "note": "device_ms: the hipEvent pair of the profile query 'dash' (upload of the job + 7 launches); call_and_download_ms: wall time "
                 "of jh_dash's host part (validation, the walk to segments, the staging copy) + the two synchronising downloads; "
                 "host_route_ms_all_paths: jl_dash_path on the first host_route_sample paths, single-threaded, minus the same number of "
                 "calls on an empty path, scaled to all paths"}
    print(json.dumps(r))
    write_json(a.out, r)
    eng.close()


if __name__ == "__main__":
    main()
