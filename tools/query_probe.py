#!/usr/bin/env python3
"""Rate of rtx_query on the headline scene against the frame that traces the
same rays.

The rays are the pixel-centre camera rays of scenes/trimesh2.ray at -w 1920
(formed as tests/test_traverse_host.py forms camera rays), resident in HBM.
After a warm-up the probe alternates, on one stream,
    query_device CLOSEST  |  query_device ALL, kmax 16  |  render_device -w 1920 -r 0
--rounds times (at least 20), each call between two stream synchronisations
with the host clock around it and device events around the queries, and
reports medians and spread.  The -r 0 frame traces the same closest-hit
queries and on top of them shades every hit and walks a shadow ray per light,
so the CLOSEST pass must not take longer than it ("closest_within_render").

Writes profiles/query_probe.json (one JSON object, also printed).
RTX_HIP_LIB selects another in-tree build of the library (recorded as "lib").
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_package():
    name = "cs378hgraphics_raytracer_amd"
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "cs378hgraphics-raytracer_amd",
                                                                     "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def build_id():
    p = os.path.join(ROOT, "cs378hgraphics-raytracer_amd", "lib", "BUILD_ID")
    return open(p).read().strip() if os.path.exists(p) else "unknown"


def camera_rays(host, width, height):
    """Pixel-centre rays (Camera::rayThrough, camera.cpp:21-31), row-major from the bottom row."""
    cam = host.desc.camera
    eye, look, u, v = (np.array(x[:]) for x in (cam.eye, cam.look, cam.u, cam.v))
    x = (np.arange(width) + 0.5) / width
    y = (np.arange(height) + 0.5) / height
    xx, yy = np.meshgrid(x, y)
    d = look[None] + (xx.reshape(-1, 1) - 0.5) * u[None] + (yy.reshape(-1, 1) - 0.5) * v[None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.repeat(eye[None], d.shape[0], 0), d


def spread(ms):
    s = sorted(ms)
    return {"ms_median": statistics.median(s), "ms_min": s[0], "ms_max": s[-1],
            "ms_p10": s[len(s) // 10], "ms_p90": s[(len(s) * 9) // 10], "samples": len(s)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default=os.path.join(ROOT, "scenes", "trimesh2.ray"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kmax", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_probe.json"))
    args = ap.parse_args()
    if args.rounds < 20:
        ap.error("--rounds must be at least 20")

    import torch

    # torch's HIP runtime first, then the library's (bench.py's order: the
    # other way round torch finds no device)
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    pkg = load_package()
    host = pkg.HostScene(args.scene)
    dev = pkg.DeviceScene(host, 0)
    height = host.height_for(args.width)
    P, D = camera_rays(host, args.width, height)
    n = P.shape[0]
    cu = torch.device("cuda:0")
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream
    dP, dD = torch.from_numpy(P).to(cu), torch.from_numpy(D).to(cu)
    out = {}
    for name, k in (("closest", 1), ("all", args.kmax)):
        out[name] = (k, torch.zeros((n, k), dtype=torch.float64, device=cu),
                     torch.zeros((n, k), dtype=torch.int32, device=cu),
                     torch.zeros((n, k), dtype=torch.int32, device=cu),
                     torch.zeros((n,), dtype=torch.int32, device=cu))
    opts = pkg.RenderOptions.from_cli(f"-w {args.width} -r 0".split())
    rgb8 = torch.zeros(n * 3, dtype=torch.uint8, device=cu)

    def query(name):
        k, t, o, f, nh = out[name]
        dev.query_device(n, dP.data_ptr(), dD.data_ptr(), name, k, t.data_ptr(), o.data_ptr(), f.data_ptr(),
                         nh.data_ptr(), stream=sp)

    def render():
        dev.render_device(opts, rgb8.data_ptr(), 0, sp)

    def timed(fn, events):
        stream.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        if events:
            e0.record(stream)
        fn()
        if events:
            e1.record(stream)
        stream.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        return wall, (e0.elapsed_time(e1) if events else None)

    for _ in range(args.warmup):
        query("closest")
        query("all")
        render()
    stream.synchronize()
    dev.frame_status()
    dev.kernel_time()  # (the launch count below: the timed renders only)
    wall = {"closest": [], "all": [], "render": []}
    evms = {"closest": [], "all": []}
    for _ in range(args.rounds):
        for name in ("closest", "all"):
            w, e = timed(lambda: query(name), True)
            wall[name].append(w)
            evms[name].append(e)
        w, _ = timed(render, False)
        wall["render"].append(w)
    dev.frame_status()
    _, launches = dev.kernel_time()

    nh_c = out["closest"][4].cpu().numpy()
    nh_a = out["all"][4].cpu().numpy()
    res = {
        "scene": os.path.basename(args.scene), "width": args.width, "height": height, "rays": n,
        "kmax": args.kmax, "rounds": args.rounds, "warmup": args.warmup,
        "build_id": build_id(), "lib": os.environ.get("RTX_HIP_LIB", "lib/librtx_hip.so"),
        "device": torch.cuda.get_device_name(0),
        "hit_share": float((nh_c > 0).mean()), "mean_list_length": float(nh_a.mean()),
        "max_list_length": int(nh_a.max()),
        "render_launches_per_frame": launches / args.rounds,
        "render_r0": spread(wall["render"]),
    }
    for name in ("closest", "all"):
        r = spread(wall[name])
        r["event_ms_median"] = statistics.median(evms[name])
        r["event_ms_min"] = min(evms[name])
        r["mrays_per_s"] = n / (r["ms_median"] * 1e-3) / 1e6
        r["mrays_per_s_event"] = n / (r["event_ms_median"] * 1e-3) / 1e6
        res[name] = r
    res["all"]["mhits_per_s"] = float(nh_a.sum()) / (res["all"]["ms_median"] * 1e-3) / 1e6
    res["closest_within_render"] = res["closest"]["ms_median"] <= res["render_r0"]["ms_median"]
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(res, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
